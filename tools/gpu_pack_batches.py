#!/usr/bin/env python3
"""What swt_pack_plan_dev + swt_pack_rows_dev cost next to two other ways of making the same arrays (needs an MI355X; DESIGN.md
4.11).

S85k-open, FastBPE ids of bench.py's 8,000-merge table, with [CLS] and [SEP]; widths 64 and 512; WHOLE and SPLIT.  Legs that
alternate round after round: plan + rows of this library (HIP events around enough back-to-back calls for 0.2 s), the plan and
the rows alone, swt_batch_rows_dev on the same ids at the same width (one sentence per row: what packing is set beside), the
same five arrays from torch ops on the device, and from NumPy on the host plus the H2D copies (wall clock).  torch and NumPy
run ONE formulation (build): next-fit by global pointer doubling, the best vectorised form there is -- a Python loop over rows
would not be a comparison.  The three constructions are compared element by element before the timing.  Prints one JSON line
per shape; --out FILE appends the lines."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_COPY_GB_S = 6290.0


def build(ids, tok_off, cmap, n_map, width, whole, sp, xp):
    """input_ids int32, mask uint8, positions, segment and sample numbers int32 [rows, width] from a sparse id stream (ids int64,
    bit 31 = continuation), with NumPy or torch"""
    kw = {} if xp is np else {"device": ids.device}
    i64 = np.int64 if xp is np else xp.int64
    search = (lambda a, v: np.searchsorted(a, v, side="right")) if xp is np else (lambda a, v: xp.searchsorted(a, v, right=True))
    n = tok_off.shape[0] - 1
    lens = tok_off[1:] - tok_off[:-1]
    body = (lens.clip(max=width - 2) if xp is np else lens.clamp(max=width - 2)) if whole else lens
    seg = body + 2
    P = xp.zeros(n + 1, dtype=i64, **kw)
    P[1:] = xp.cumsum(seg, 0)
    total = int(P[-1])
    if whole:
        # next(r), the node n its own successor; the orbit of 0 marked through the doubling tables from the longest jump down
        nxt = search(P, P[:-1] + width) - 1
        jump = xp.zeros(n + 1, dtype=i64, **kw)
        jump[:n], jump[n] = nxt, n
        jumps = [jump]
        while (1 << len(jumps)) < n + 1:
            jumps.append(jumps[-1][jumps[-1]])
        mark = xp.zeros(n + 1, dtype=xp.bool_ if xp is np else xp.bool, **kw)
        mark[0] = True
        for j in reversed(jumps):
            mark[j[mark]] = True
        mark[n] = False
        starts = xp.nonzero(mark)[0] if xp is np else xp.nonzero(mark)[:, 0]
        rows = int(starts.shape[0])
        row_at = P[starts]                                        # the stream position of every packed row's column 0
        ends = xp.zeros(rows, dtype=i64, **kw)
        ends[:-1], ends[-1] = row_at[1:], total
        owner = starts
    else:
        rows = -(-total // width)
        row_at = xp.arange(rows, dtype=i64, **kw) * width
        ends = (row_at + width).clip(max=total) if xp is np else (row_at + width).clamp(max=total)
        owner = search(P[1:], row_at)
    col = xp.arange(width, dtype=i64, **kw)
    x = row_at[:, None] + col[None, :]
    live = x < ends[:, None]
    r = search(P[1:], x.reshape(-1)).reshape(rows, width)
    r = r.clip(max=n - 1) if xp is np else r.clamp(max=n - 1)
    p = x - P[r]
    idx = tok_off[:-1][r] + p - 1
    idx = idx.clip(0, ids.shape[0] - 1) if xp is np else idx.clamp(0, ids.shape[0] - 1)
    raw = ids[idx]
    dense = cmap[(raw & 0x7FFFFFFF) + (raw >> 31) * n_map]
    dense = xp.where(dense == 0xFFFFFFFF, xp.full_like(dense, sp["unk"]), dense)
    out = xp.where(p == 0, xp.full_like(dense, sp["cls"]), dense)
    out = xp.where(p == seg[r] - 1, xp.full_like(dense, sp["sep"]), out)
    out = xp.where(live, out, xp.full_like(dense, sp["pad"]))
    minus = xp.full_like(p, -1)
    res = (out, live, xp.where(live, p, xp.zeros_like(p)), xp.where(live, r - owner[:, None], minus), xp.where(live, r, minus))
    if xp is np:
        return tuple(a.astype(np.uint8 if k == 1 else np.int32) for k, a in enumerate(res))
    return tuple(a.to(xp.uint8 if k == 1 else xp.int32) for k, a in enumerate(res))


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

    N.init(0)
    tok = tokenizers.FastBPE()
    tok.merges_list = list(synth.pretrained_merges()[:8000])
    tok._build_table()
    voc = tok._batch_vocabulary()
    sp = tok.special_ids()
    sents = synth.s85k_open(args.sentences)
    h_ids, h_off = tok.encode_ids_batch(sents)
    n_tok, n_rows = int(h_ids.size), len(sents)
    d_ids = torch.from_numpy(np.concatenate([h_ids, np.zeros(4, np.uint32)]).view(np.int32)).cuda()
    d_off = torch.from_numpy(h_off.view(np.int64)).cuda()
    d_map = torch.from_numpy(voc.cmap.view(np.int32)).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    lib = N.lib()
    t_ids, t_map = (d_ids[:n_tok].to(torch.int64) & 0xFFFFFFFF), (d_map.to(torch.int64) & 0xFFFFFFFF)
    n_ids, n_map64, n_off = h_ids.astype(np.int64), voc.cmap.astype(np.int64), h_off.astype(np.int64)
    lines = []
    for width in (64, 512):
        for name, mode in (("whole", N.PACK_WHOLE), ("split", N.PACK_SPLIT)):
            spec = N.batch_spec(width, 0, False, False, False, sp["pad"], sp["unk"], sp["cls"], sp["sep"])
            d_slot, d_first = (torch.empty(n_rows + 1, dtype=torch.int64, device="cuda") for _ in range(2))
            d_info = torch.zeros(4, dtype=torch.int64, device="cuda")

            def plan():
                N.check(lib.swt_pack_plan_dev(d_off.data_ptr(), n_rows, C.byref(spec), mode, d_slot.data_ptr(), d_first.data_ptr(),
                                              d_info.data_ptr(), stream))

            plan()
            pinfo = d_info.cpu().numpy()
            rows, longest, total = int(pinfo[0]), int(pinfo[1]), int(pinfo[3])
            o = [torch.empty((rows, width), dtype=torch.uint8 if k == 1 else torch.int32, device="cuda") for k in range(5)]
            o_len, d_rinfo = torch.empty(rows, dtype=torch.int32, device="cuda"), torch.zeros(4, dtype=torch.int64, device="cuda")
            one_ids, one_mask = torch.empty((n_rows, width), dtype=torch.int32, device="cuda"), torch.empty((n_rows, width), dtype=torch.uint8, device="cuda")

            def rows_call():
                N.check(lib.swt_pack_rows_dev(d_ids.data_ptr(), d_off.data_ptr(), n_rows, d_map.data_ptr(), voc.n_map, 1, C.byref(spec), mode,
                                              d_slot.data_ptr(), d_first.data_ptr(), rows, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(),
                                              o[3].data_ptr(), o[4].data_ptr(), o_len.data_ptr(), d_rinfo.data_ptr(), stream))

            def ours():
                plan()
                rows_call()

            def one_per_row():
                N.check(lib.swt_batch_rows_dev(d_ids.data_ptr(), d_off.data_ptr(), n_rows, d_map.data_ptr(), voc.n_map, 1, None, None,
                                               C.byref(spec), None, n_rows, one_ids.data_ptr(), one_mask.data_ptr(), None, None, None, None,
                                               d_rinfo.data_ptr(), stream))

            def by_torch():
                return build(t_ids, d_off, t_map, voc.n_map, width, mode == N.PACK_WHOLE, sp, torch)

            def by_numpy():
                return tuple(torch.from_numpy(a).cuda() for a in build(n_ids, n_off, n_map64, voc.n_map, width, mode == N.PACK_WHOLE, sp, np))

            ours()
            torch.cuda.synchronize()
            rinfo = d_rinfo.cpu().numpy()
            for leg, other in (("torch_device", by_torch()), ("numpy_host", by_numpy())):
                for what, a, b in zip(("input_ids", "attention_mask", "position_ids", "sequence_ids", "sample_ids"), other, o):
                    if a.shape != b.shape or not torch.equal(a, b):
                        bad = (a != b).nonzero()[:3].tolist() if a.shape == b.shape else []
                        raise AssertionError("%s of %s differs from swt_pack_rows_dev: shapes %s %s, first at %s: %s" % (
                            what, leg, tuple(a.shape), tuple(b.shape), bad, [(int(a[i, j]), int(b[i, j])) for i, j in bad]))

            def timed(fn, reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    fn()
                e1.record(); e1.synchronize()
                return e0.elapsed_time(e1) / reps

            device_legs = {"pack_plan_and_rows_dev": ours, "pack_plan_dev": plan, "pack_rows_dev": rows_call, "batch_rows_dev_one_per_row": one_per_row}
            reps = {k: max(1, int(np.ceil(250.0 / max(timed(fn, 50), 1e-3)))) for k, fn in device_legs.items()}
            ms = {k: [] for k in list(device_legs) + ["torch_device", "numpy_host"]}
            for r in range(args.warmup + args.rounds):
                t = {k: timed(fn, reps[k]) for k, fn in device_legs.items()}
                t["torch_device"] = timed(by_torch, 1)
                torch.cuda.synchronize()
                t0 = time.perf_counter(); by_numpy(); torch.cuda.synchronize()
                t["numpy_host"] = (time.perf_counter() - t0) * 1e3
                if r >= args.warmup:
                    for k, v in t.items():
                        ms[k].append(v)
            live = int(o_len.to(torch.int64).sum().item())
            tokens_read = live - 2 * n_rows  # every segment has its [CLS] and [SEP]
            read_b = 8 * tokens_read + 16 * n_rows + 16 * n_rows  # ids and map entries; offsets; slot and row_first
            write_b = 17 * rows * width + 4 * rows                 # ids, mask, positions, segments, samples; lengths
            out = {"shape": "%s_%d" % (name, width), "corpus": "S85k-open", "sentences": n_rows, "tokens": n_tok, "longest_row": longest,
                   "width": width, "mode": name, "rows_out": rows, "columns": total, "density": round(min(total, rows * width) / (rows * width), 4),
                   "density_one_per_row": round(float((torch.clamp(d_off[1:] - d_off[:-1], max=width - 2) + 2).sum().item()) / (n_rows * width), 4),
                   "rows_that_lost_tokens": int(rinfo[1]), "tokens_to_unk": int(rinfo[2]), "calls_per_window": reps, "rounds": args.rounds,
                   "bytes_read_rows": read_b, "bytes_written_rows": write_b, "legs": {}}
            for leg, v in ms.items():
                med = statistics.median(v)
                out["legs"][leg] = {"ms": [round(x, 4) for x in v], "median_ms": round(med, 4), "spread": round((max(v) - min(v)) / med, 4)}
            med = out["legs"]["pack_plan_and_rows_dev"]["median_ms"]
            rows_med = out["legs"]["pack_rows_dev"]["median_ms"]
            out["rows_gb_s"] = round((read_b + write_b) / 1e6 / rows_med, 1)
            out["rows_share_of_hbm_copy"] = round(out["rows_gb_s"] / HBM_COPY_GB_S, 4)
            for leg in ("torch_device", "numpy_host"):
                out["legs"][leg]["ratio_to_pack_plan_and_rows_dev"] = round(out["legs"][leg]["median_ms"] / med, 1)
            lines.append(json.dumps(out))
            print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a", encoding="utf-8") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
