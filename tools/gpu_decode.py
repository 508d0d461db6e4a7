#!/usr/bin/env python3
"""What swt_decode_plan_dev + swt_decode_rows_dev cost next to torch ops that make the same bytes (needs an MI355X).

S85k-open, FastBPE ids of bench.py's 8,000-merge table with [CLS] and [SEP]: one sentence per row at width 64, and packed
"whole" at width 512.  The library's text, offsets, status and info are compared with the Python model of the tests first, the
torch leg's bytes too.  Then legs that alternate round after round, HIP events around enough back-to-back calls for 0.2 s:
plan + rows of the library, and the same bytes from torch ops on the device (flags and lengths gathered, the previous kept
column by cummax, cumsum, repeat_interleave, a byte gather); neither leg reads anything back between its launches (both are
given the total).  Once, for scale, the Python model on the CPU.  Prints one JSON line per shape; --out FILE appends the lines."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_COPY_GB_S = 6290.0


def by_torch(torch, ids, mask, d_bytes, d_off, d_flags, total):
    """-> (text uint8[total], text_off int64[rows + 1]) with torch ops on the device, skip_special_tokens on"""
    rows, width = ids.shape
    idx = ids.to(torch.int64)
    f = d_flags[idx].to(torch.int32)
    kept = (mask != 0) & ((f & 8) == 0)
    col = torch.arange(width, device=ids.device, dtype=torch.int64).expand(ids.shape)
    last = torch.cummax(torch.where(kept, col, torch.full_like(col, -1)), dim=1).values
    prev = torch.nn.functional.pad(last[:, :-1], (1, 0), value=-1)
    has_prev = prev >= 0
    pf = torch.gather(f, 1, prev.clamp(min=0))
    glue = has_prev & ((f & 1) != 0)
    space = has_prev & ~glue & ((f & 2) == 0) & ((pf & 4) == 0)
    start = d_off[idx].to(torch.int64)
    nb = d_off[idx + 1].to(torch.int64) - start
    length = torch.where(kept, nb - 2 * glue.to(torch.int64) + space.to(torch.int64), torch.zeros_like(nb))
    flat = length.reshape(-1)
    ends = torch.cumsum(flat, 0)
    text_off = torch.nn.functional.pad(ends.reshape(rows, width)[:, -1], (1, 0))
    cell = torch.repeat_interleave(torch.arange(flat.numel(), device=ids.device), flat, output_size=total)
    k = torch.arange(total, device=ids.device, dtype=torch.int64) - (ends - flat)[cell]
    sp = space.reshape(-1)[cell]
    src = start.reshape(-1)[cell] + 2 * glue.reshape(-1)[cell].to(torch.int64) + k - sp.to(torch.int64)
    text = torch.where(sp & (k == 0), torch.full((), 32, dtype=torch.uint8, device=ids.device), d_bytes[src.clamp(min=0)])
    return text, text_off


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
    from tests import decode_cases as D

    N.init(0)
    tok = tokenizers.FastBPE()
    tok.merges_list = list(synth.pretrained_merges()[:8000])
    tok._build_table()
    voc = tok._batch_vocabulary()
    tabs = voc.decode_tables
    tok_bytes, tok_off, tok_flags, n_tok = tabs
    sents = synth.s85k_open(args.sentences)
    stream = torch.cuda.current_stream().cuda_stream
    lib = N.lib()
    d_bytes, d_off = torch.from_numpy(tok_bytes.copy()).cuda(), torch.from_numpy(tok_off.view(np.int32)).cuda()
    d_flags = torch.from_numpy(tok_flags).cuda()
    shapes = (("one_per_row_64", {"max_length": 64, "padding": "max_length"}), ("whole_512", {"max_length": 512, "packing": "whole"}))
    lines = []
    for name, kw in shapes:
        enc = tok.encode_batch(sents, device=True, **kw)
        ids, mask = enc["input_ids"].contiguous(), enc["attention_mask"].contiguous()
        rows, width = (int(x) for x in ids.shape)
        flags = N.DECODE_SKIP_SPECIAL | (N.DECODE_IDS64 if ids.dtype == torch.int64 else 0)
        d_text_off = torch.empty(rows + 1, dtype=torch.int64, device="cuda")
        d_status, d_info = torch.empty(rows, dtype=torch.uint8, device="cuda"), torch.zeros(3, dtype=torch.int64, device="cuda")
        head = (ids.data_ptr(), mask.data_ptr(), rows, width)

        def plan():
            N.check(lib.swt_decode_plan_dev(*head, d_off.data_ptr(), d_flags.data_ptr(), n_tok, flags, d_text_off.data_ptr(), d_status.data_ptr(),
                                            d_info.data_ptr(), stream))

        plan()
        total = int(d_info.cpu()[0])
        d_text = torch.empty(total, dtype=torch.uint8, device="cuda")

        def write():
            N.check(lib.swt_decode_rows_dev(*head, d_bytes.data_ptr(), d_off.data_ptr(), d_flags.data_ptr(), n_tok, flags, d_text_off.data_ptr(),
                                            d_text.data_ptr(), total, stream))

        write()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        want = D.decode(ids.cpu().numpy(), mask.cpu().numpy(), tabs, D.SKIP_SPECIAL)
        model_s = time.perf_counter() - t0
        for what, a, b in (("text", d_text, want[0]), ("text_off", d_text_off, want[1].view(np.int64)), ("status", d_status, want[2]),
                           ("info", d_info, want[3].view(np.int64))):
            if not np.array_equal(a.cpu().numpy(), b):
                raise AssertionError("%s: %s of swt_decode_*_dev differs from the model" % (name, what))
        t_text, t_off = by_torch(torch, ids, mask, d_bytes, d_off, d_flags, total)
        if not np.array_equal(t_text.cpu().numpy(), want[0]) or not np.array_equal(t_off.cpu().numpy(), want[1].view(np.int64)):
            raise AssertionError("%s: the torch leg differs from the model" % name)
        del t_text, t_off

        def timed(fn, reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record(); e1.synchronize()
            return e0.elapsed_time(e1) / reps

        legs = {"decode_dev": lambda: (plan(), write()), "decode_plan_dev": plan, "decode_rows_dev": write,
                "torch": lambda: by_torch(torch, ids, mask, d_bytes, d_off, d_flags, total)}
        reps = {k: max(1, int(np.ceil(200.0 / max(timed(fn, 10), 1e-3)))) for k, fn in legs.items()}
        ms = {k: [] for k in legs}
        for r in range(args.warmup + args.rounds):
            t = {k: timed(fn, reps[k]) for k, fn in legs.items()}
            if r >= args.warmup:
                for k, v in t.items():
                    ms[k].append(v)
        cells, size = rows * width, ids.element_size()
        must = cells * (size + 1) + total + 8 * (rows + 1)  # ids and mask once, the text and its offsets once; the tables stay in L2
        out = {"shape": name, "corpus": "S85k-open", "sentences": len(sents), "rows": rows, "width": width,
               "id_bytes": size, "text_bytes": total, "kept_columns": int(want[3][2]), "vocabulary_bytes": int(tok_off[-1]), "tokens": n_tok,
               "bytes_must_move": must, "calls_per_window": reps, "rounds": args.rounds, "python_model_s": round(model_s, 2), "legs": {}}
        for leg, v in ms.items():
            med = statistics.median(v)
            out["legs"][leg] = {"ms": [round(x, 4) for x in v], "median_ms": round(med, 4), "spread": round((max(v) - min(v)) / med, 4)}
        out["legs"]["decode_dev"]["gb_s"] = round(must / 1e6 / out["legs"]["decode_dev"]["median_ms"], 1)
        out["legs"]["decode_dev"]["share_of_hbm_copy"] = round(out["legs"]["decode_dev"]["gb_s"] / HBM_COPY_GB_S, 4)
        out["legs"]["torch"]["ratio_to_decode_dev"] = round(out["legs"]["torch"]["median_ms"] / out["legs"]["decode_dev"]["median_ms"], 1)
        lines.append(json.dumps(out))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a", encoding="utf-8") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
