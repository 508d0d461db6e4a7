#!/usr/bin/env python3
"""What swt_batch_rows_dev costs next to two other ways of making the same arrays (needs an MI355X).

S85k-open, FastBPE ids of bench.py's 8,000-merge table, width 64 with [CLS] and [SEP]: truncating, and windowed with stride 8.
Three legs alternate round after round: swt_batch_rows_dev (HIP events around enough back-to-back calls for 0.2 s), the same
arrays from torch ops on the device, and from NumPy on encode_ids_batch's host arrays plus the H2D copy (wall clock).  The three
results are compared before the timing.  Prints one JSON line per shape: per leg the times, median and spread; the bytes the new
path reads and writes by the shapes, its GB/s and the share of the 6.29 TB/s a copy reaches.  --out FILE appends the lines."""
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
WIDTH = 64


def rows_of(lens, cap, step, windows, xp):
    """-> (sample, first token inside the sample, body length) per output row, with NumPy or torch"""
    n = lens.shape[0]
    if not windows:
        k = xp.ones_like(lens)
    else:
        k = xp.where(lens <= cap, xp.ones_like(lens), 1 + (lens - cap + step - 1) // step)
    base = xp.cumsum(k, 0) - k
    if xp is np:
        sample = np.repeat(np.arange(n, dtype=np.int64), k)
        w = np.arange(sample.shape[0], dtype=np.int64) - base[sample]
        body = np.minimum(lens[sample] - w * step, cap)
    else:
        sample = xp.repeat_interleave(xp.arange(n, device=lens.device), k)
        w = xp.arange(sample.shape[0], device=lens.device) - base[sample]
        body = xp.clamp(lens[sample] - w * step, max=cap)
    return sample, w * step, body


def build(ids, tok_off, cmap, n_map, cap, step, windows, sp, xp):
    """input_ids int32[rows, WIDTH] and the mask uint8, from a sparse id stream: ids int64 (bit 31 = continuation)"""
    lens = tok_off[1:] - tok_off[:-1]
    sample, first, body = rows_of(lens, cap, step, windows, xp)
    col = xp.arange(WIDTH) if xp is np else xp.arange(WIDTH, device=ids.device)
    p = col[None, :] - 1
    live = (p >= 0) & (p < body[:, None])
    idx = (tok_off[:-1][sample] + first)[:, None] + p
    idx = idx.clip(0, ids.shape[0] - 1) if xp is np else idx.clamp(0, ids.shape[0] - 1)
    raw = ids[idx]
    dense = cmap[(raw & 0x7FFFFFFF) + (raw >> 31) * n_map]
    dense = xp.where(dense == 0xFFFFFFFF, xp.full_like(dense, sp["unk"]), dense)  # (every id of this stream lies inside the map)
    out = xp.where(live, dense, sp["pad"])
    out[:, 0] = sp["cls"]
    rows = xp.arange(out.shape[0]) if xp is np else xp.arange(out.shape[0], device=ids.device)
    out[rows, body + 1] = sp["sep"]
    mask = col[None, :] < (body + 2)[:, None]
    if xp is np:
        return out.astype(np.int32), mask.astype(np.uint8)
    return out.to(xp.int32), mask.to(xp.uint8)


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
    # what the comparisons index with: ids and map as int64, made once outside the timing (the host ones likewise)
    t_ids, t_map = (d_ids[:n_tok].to(torch.int64) & 0xFFFFFFFF), (d_map.to(torch.int64) & 0xFFFFFFFF)
    n_ids, n_map64, n_off = h_ids.astype(np.int64), voc.cmap.astype(np.int64), h_off.astype(np.int64)
    lines = []
    for name, windows, stride in (("truncate", False, 0), ("windows_stride8", True, 8)):
        spec = N.batch_spec(WIDTH, stride, windows, False, False, sp["pad"], sp["unk"], sp["cls"], sp["sep"])
        cap, step = WIDTH - 2, WIDTH - 2 - stride
        d_base, d_info = torch.empty(n_rows + 1, dtype=torch.int64, device="cuda"), torch.zeros(4, dtype=torch.int64, device="cuda")
        N.check(lib.swt_batch_plan_dev(d_off.data_ptr(), n_rows, C.byref(spec), d_base.data_ptr(), d_info.data_ptr(), stream))
        rows, longest = int(d_info[0].item()), int(d_info[1].item())
        o_ids = torch.empty((rows, WIDTH), dtype=torch.int32, device="cuda")
        o_mask = torch.empty((rows, WIDTH), dtype=torch.uint8, device="cuda")
        o_sample, o_len = torch.empty(rows, dtype=torch.int32, device="cuda"), torch.empty(rows, dtype=torch.int32, device="cuda")

        def ours():
            N.check(lib.swt_batch_rows_dev(d_ids.data_ptr(), d_off.data_ptr(), n_rows, d_map.data_ptr(), voc.n_map, 1, None, None, C.byref(spec),
                                           d_base.data_ptr() if windows else None, rows, o_ids.data_ptr(), o_mask.data_ptr(), None, None,
                                           o_sample.data_ptr(), o_len.data_ptr(), d_info.data_ptr(), stream))

        def by_torch():
            return build(t_ids, d_off, t_map, voc.n_map, cap, step, windows, sp, torch)

        def by_numpy():
            a, m = build(n_ids, n_off, n_map64, voc.n_map, cap, step, windows, sp, np)
            return torch.from_numpy(a).cuda(), torch.from_numpy(m).cuda()

        ours()
        torch.cuda.synchronize()
        info = d_info.cpu().numpy()
        for leg, other in (("torch_device", by_torch()), ("numpy_host", by_numpy())):
            for what, a, b in (("input_ids", other[0], o_ids), ("attention_mask", other[1], o_mask)):
                if a.shape != b.shape or not torch.equal(a, b):
                    bad = (a != b).nonzero()[:3].tolist() if a.shape == b.shape else []
                    raise AssertionError("%s of %s differs from swt_batch_rows_dev: shapes %s %s, first at %s: %s" % (
                        what, leg, tuple(a.shape), tuple(b.shape), bad, [(int(a[i, j]), int(b[i, j])) for i, j in bad]))
        # back-to-back calls of the new path for a window of at least 0.2 s, sized from one timed call
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(100):
            ours()
        e1.record(); e1.synchronize()
        reps = max(1, int(np.ceil(250.0 / max(e0.elapsed_time(e1) / 100, 1e-3))))
        ms = {"batch_rows_dev": [], "torch_device": [], "numpy_host": []}
        for r in range(args.warmup + args.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                ours()
            e1.record(); e1.synchronize()
            t_ours = e0.elapsed_time(e1) / reps
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); by_torch(); e1.record(); e1.synchronize()
            t_torch = e0.elapsed_time(e1)
            torch.cuda.synchronize()
            t0 = time.perf_counter(); by_numpy(); torch.cuda.synchronize()
            t_numpy = (time.perf_counter() - t0) * 1e3
            if r >= args.warmup:
                ms["batch_rows_dev"].append(t_ours); ms["torch_device"].append(t_torch); ms["numpy_host"].append(t_numpy)
        slots_live = int(o_len.to(torch.int64).sum().item()) - 2 * rows  # token slots read, the overlap of the windows counted again
        read_b, write_b = 8 * slots_live + 16 * n_rows, 5 * rows * WIDTH + 8 * rows
        out = {"shape": name, "corpus": "S85k-open", "sentences": n_rows, "tokens": n_tok, "longest_row": longest, "width": WIDTH,
               "stride": stride, "rows_out": rows, "rows_that_lost_tokens": int(info[1]), "tokens_to_unk": int(info[2]),
               "calls_per_window": reps, "rounds": args.rounds, "bytes_read": read_b, "bytes_written": write_b, "legs": {}}
        for leg, v in ms.items():
            med = statistics.median(v)
            out["legs"][leg] = {"ms": [round(x, 4) for x in v], "median_ms": round(med, 4), "spread": round((max(v) - min(v)) / med, 4)}
        med = out["legs"]["batch_rows_dev"]["median_ms"]
        out["window_s"] = round(med * reps / 1e3, 3)
        out["gb_s"] = round((read_b + write_b) / 1e6 / med, 1)
        out["share_of_hbm_copy"] = round(out["gb_s"] / HBM_COPY_GB_S, 4)
        for leg in ("torch_device", "numpy_host"):
            out["legs"][leg]["ratio_to_batch_rows_dev"] = round(out["legs"][leg]["median_ms"] / med, 1)
        lines.append(json.dumps(out))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a", encoding="utf-8") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
