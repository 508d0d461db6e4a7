#!/usr/bin/env python3
"""What swt_batch_pair_rows_dev costs next to the same arrays composed from torch ops on the device (needs an MI355X; DESIGN.md
4.10).

The common question-answering shape: S85k-open's first sentences as questions, a second slice of the same corpus -- SPAN
sentences in a row per context, through a second offset array into the one id stream -- as contexts; FastBPE ids of bench.py's
8,000-merge table; width 384 with [CLS] and both [SEP], only_second: truncating, and windowed with stride 128.  Two legs
alternate round after round: swt_batch_pair_rows_dev (HIP events around enough back-to-back calls for 0.25 s) and input_ids,
attention_mask, token_type_ids, special_tokens_mask and sequence_ids from torch ops.  The results are compared before the timing.
Prints one JSON line per shape: per leg the times, median and spread; the bytes the pair kernel reads and writes by the shapes,
its GB/s and the share of the 6.29 TB/s a copy reaches.  --out FILE appends the lines."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_COPY_GB_S = 6290.0
WIDTH, STRIDE, SPAN = 384, 128, 12
NAMES = ("input_ids", "attention_mask", "token_type_ids", "special_tokens_mask", "sequence_ids")


def build(torch, ids, off_a, off_b, cmap, n_map, windows, sp):
    """the five per-column arrays of only_second from a sparse id stream (ids int64, bit 31 = continuation); no pair is refused"""
    cap = WIDTH - 3
    la, lb = off_a[1:] - off_a[:-1], off_b[1:] - off_b[:-1]
    budget = cap - la
    step = budget - STRIDE
    one = torch.ones_like(la)
    k = torch.where(lb <= budget, one, 1 + (lb - budget + step - 1) // step) if windows else one
    base = torch.cumsum(k, 0) - k
    sample = torch.repeat_interleave(torch.arange(la.shape[0], device=ids.device), k)
    first = (torch.arange(sample.shape[0], device=ids.device) - base[sample]) * step[sample]
    la_s = la[sample][:, None]
    lb_s = torch.minimum(lb[sample] - first, budget[sample])[:, None]
    p = torch.arange(WIDTH, device=ids.device)[None, :]
    in_a, in_b = (p >= 1) & (p <= la_s), (p >= la_s + 2) & (p < la_s + 2 + lb_s)
    idx = torch.where(in_a, off_a[:-1][sample][:, None] + p - 1, (off_b[:-1][sample] + first)[:, None] + p - la_s - 2)
    raw = ids[idx.clamp(0, ids.shape[0] - 1)]
    dense = cmap[(raw & 0x7FFFFFFF) + (raw >> 31) * n_map]
    dense = torch.where(dense == 0xFFFFFFFF, torch.full_like(dense, sp["unk"]), dense)
    token = in_a | in_b
    out = torch.where(token, dense, sp["pad"])
    out[:, 0] = sp["cls"]
    out = torch.where((p == la_s + 1) | (p == la_s + 2 + lb_s), sp["sep"], out)
    live = p <= la_s + 2 + lb_s
    seq = torch.where(in_a, 0, torch.where(in_b, 1, -1))
    return (out.to(torch.int32), live.to(torch.uint8), ((p >= la_s + 2) & live).to(torch.int32), (~token).to(torch.uint8), seq.to(torch.int8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
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
    voc = tok._batch_vocabulary()
    sp = tok.special_ids()
    n = args.pairs
    sents = synth.s85k_open(n * (1 + SPAN))
    h_ids, h_off = tok.encode_ids_batch(sents)
    h_off = h_off.astype(np.int64)
    h_a, h_b = h_off[:n + 1].copy(), h_off[n::SPAN].copy()  # context i: the sentences n + SPAN i .. n + SPAN (i + 1) - 1
    assert h_b.size == n + 1
    n_tok = int(h_ids.size)
    d_ids = torch.from_numpy(np.concatenate([h_ids, np.zeros(4, np.uint32)]).view(np.int32)).cuda()
    d_a, d_b = torch.from_numpy(h_a).cuda(), torch.from_numpy(h_b).cuda()
    d_map = torch.from_numpy(voc.cmap.view(np.int32)).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    lib = N.lib()
    t_ids, t_map = (d_ids[:n_tok].to(torch.int64) & 0xFFFFFFFF), (d_map.to(torch.int64) & 0xFFFFFFFF)  # what the torch leg indexes with
    lines = []
    for name, windows in (("truncate", False), ("windows_stride128", True)):
        spec = N.batch_spec(WIDTH, STRIDE, windows, False, False, sp["pad"], sp["unk"], sp["cls"], sp["sep"])
        d_base, d_status = torch.empty(n + 1, dtype=torch.int64, device="cuda"), torch.empty(n + 8, dtype=torch.uint8, device="cuda")
        d_info = torch.zeros(8, dtype=torch.int64, device="cuda")
        N.check(lib.swt_batch_pair_plan_dev(d_a.data_ptr(), d_b.data_ptr(), n, C.byref(spec), N.PAIR_ONLY_SECOND, d_base.data_ptr(),
                                            d_status.data_ptr(), d_info.data_ptr(), stream))
        plan = d_info.cpu().numpy()
        rows, longest = int(plan[0]), int(plan[1])
        if plan[3]:
            raise AssertionError("%d refused pairs: the torch leg does not make their rows" % int(plan[3]))
        o = {k: torch.empty((rows, WIDTH), dtype=dt, device="cuda") for k, dt in zip(NAMES, (torch.int32, torch.uint8, torch.int32, torch.uint8, torch.int8))}
        o_sample, o_len = torch.empty(rows, dtype=torch.int32, device="cuda"), torch.empty(rows, dtype=torch.int32, device="cuda")

        def ours():
            N.check(lib.swt_batch_pair_rows_dev(d_ids.data_ptr(), d_a.data_ptr(), d_b.data_ptr(), n, d_map.data_ptr(), voc.n_map, 1, None, None,
                                                C.byref(spec), N.PAIR_ONLY_SECOND, d_base.data_ptr() if windows else None, d_status.data_ptr(),
                                                rows, o[NAMES[0]].data_ptr(), o[NAMES[1]].data_ptr(), o[NAMES[2]].data_ptr(),
                                                o[NAMES[3]].data_ptr(), o[NAMES[4]].data_ptr(), None, None, o_sample.data_ptr(),
                                                o_len.data_ptr(), d_info.data_ptr(), stream))

        def by_torch():
            return build(torch, t_ids, d_a, d_b, t_map, voc.n_map, windows, sp)

        ours()
        torch.cuda.synchronize()
        info = d_info.cpu().numpy()
        for what, a in zip(NAMES, by_torch()):
            b = o[what]
            if a.shape != b.shape or not torch.equal(a, b):
                bad = (a != b).nonzero()[:3].tolist() if a.shape == b.shape else []
                raise AssertionError("%s of the torch ops differs from swt_batch_pair_rows_dev: shapes %s %s, first at %s: %s" % (
                    what, tuple(a.shape), tuple(b.shape), bad, [(int(a[i, j]), int(b[i, j])) for i, j in bad]))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(50):
            ours()
        e1.record(); e1.synchronize()
        reps = max(1, int(np.ceil(250.0 / max(e0.elapsed_time(e1) / 50, 1e-3))))
        ms = {"pair_rows_dev": [], "torch_device": []}
        for r in range(args.warmup + args.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                ours()
            e1.record(); e1.synchronize()
            t_ours = e0.elapsed_time(e1) / reps
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); by_torch(); e1.record(); e1.synchronize()
            if r >= args.warmup:
                ms["pair_rows_dev"].append(t_ours); ms["torch_device"].append(e0.elapsed_time(e1))
        slots_live = int(o_len.to(torch.int64).sum().item()) - 3 * rows  # token slots read; the question once per window
        read_b, write_b = 8 * slots_live + 40 * n, 11 * rows * WIDTH + 8 * rows
        out = {"shape": name, "corpus": "S85k-open", "pairs": n, "sentences_per_context": SPAN, "tokens": n_tok, "largest_pair": longest,
               "width": WIDTH, "stride": STRIDE if windows else 0, "strategy": "only_second", "rows_out": rows, "pairs_that_lost_tokens": int(info[4]),
               "tokens_to_unk": int(info[2]), "calls_per_window": reps, "rounds": args.rounds, "bytes_read": read_b, "bytes_written": write_b,
               "legs": {}}
        for leg, v in ms.items():
            med = statistics.median(v)
            out["legs"][leg] = {"ms": [round(x, 4) for x in v], "median_ms": round(med, 4), "spread": round((max(v) - min(v)) / med, 4)}
        med = out["legs"]["pair_rows_dev"]["median_ms"]
        out["window_s"] = round(med * reps / 1e3, 3)
        out["gb_s"] = round((read_b + write_b) / 1e6 / med, 1)
        out["share_of_hbm_copy"] = round(out["gb_s"] / HBM_COPY_GB_S, 4)
        out["legs"]["torch_device"]["ratio_to_pair_rows_dev"] = round(out["legs"]["torch_device"]["median_ms"] / med, 1)
        lines.append(json.dumps(out))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a", encoding="utf-8") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
