#!/usr/bin/env python3
"""What the NaiveBPE batch path costs next to FastBPE's (needs an MI355X; reads nothing but the package).

S85k-open resident in HBM, the 8,000-merge table of bench.py's encode config, K timed steps per leg after W warm-up steps, the
region bracketed by a device synchronisation on both sides (bench.py's encode_corpus_bench), each leg repeated R times:

  a  swt_bpe_encode_dev                                   the FastBPE path
  b  swt_bpe_encode_naive_dev on the same table           order-equivalent: must launch the same kernels as a
  c  swt_bpe_encode_naive_dev on the table with two       not order-equivalent: the ordered form of bpe_lane_kernel
     dependent merges swapped
  d  swt_bpe_encode_dev on the table of c                 FastBPE on an improper table (the literal rounds), for scale

Prints one JSON line: ms per step of every repeat, median, spread ((max - min) / median), the ratios to a, the time of the
dominant kernel alone, and whether b's output equals a's.  --leg a|b|c|d runs ONE leg once without the timing (for a kernel trace).

--parent-lib FILE loads the parent commit's libswt_hip.so beside this tree's and adds "against_parent": legs c and d through both
libraries on the same table, alternating repeat after repeat in this one process, the ids compared first.  A leg passes when this
tree's median does not exceed the parent's by more than the parent's own spread (max - min) in this run.
"""
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


def swap_dependent(merges, at):
    """two merges swapped of which the second uses what the first produces: the list is not proper any more"""
    merges = list(merges)
    for i in range(at, len(merges)):
        made = merges[i][0] + merges[i][1]
        for j in range(i + 1, len(merges)):
            if made in merges[j]:
                merges[i], merges[j] = merges[j], merges[i]
                return merges, (i, j)
    raise SystemExit("no dependent pair of merges")


def against_parent(args, N, torch, bad, step, result, call_args):
    """legs c and d through this tree's library and the parent's, alternating"""
    d_text, n_bytes, d_off, n_sent, d_out, d_out_off, d_ntok, stream = call_args
    parent = C.CDLL(os.path.abspath(args.parent_lib))
    entries = {"c": "swt_bpe_encode_naive_dev", "d": "swt_bpe_encode_dev"}
    for name in ("swt_init", "swt_last_error", "swt_bpe_table_create", "swt_bpe_table_destroy") + tuple(entries.values()):
        fn = getattr(parent, name)
        fn.restype, fn.argtypes = N.SIGNATURES[name]
    if parent.swt_init(0):
        raise RuntimeError("the parent's library does not initialise")
    syms = type(bad._naive_syms)()
    tri = np.array([x for l, r in bad.merges_list for x in (syms.intern(l), syms.intern(r), syms.intern(l + r))], dtype=np.uint32).reshape(-1, 3)
    left, right, merged = (np.ascontiguousarray(tri[:, k]) for k in range(3))
    h = C.c_void_p()
    if parent.swt_bpe_table_create(N.ptr(left, N.u32p), N.ptr(right, N.u32p), N.ptr(merged, N.u32p), len(left), C.byref(h)):
        raise RuntimeError("the parent's table: %s" % parent.swt_last_error().decode())

    def parent_step(leg):
        rc = getattr(parent, entries[leg])(h, d_text.data_ptr(), n_bytes, d_off.data_ptr(), n_sent, d_out.data_ptr(), d_out_off.data_ptr(),
                                           d_ntok.data_ptr(), 0, stream)
        if rc:
            raise RuntimeError("%s (parent): %d %s" % (entries[leg], rc, parent.swt_last_error().decode()))

    runs = {"c": lambda: step("c"), "c_parent": lambda: parent_step("c"), "d": lambda: step("d"), "d_parent": lambda: parent_step("d")}
    for leg in "cd":  # the same ids from both libraries, before any timing
        here = result(leg)
        parent_step(leg)
        torch.cuda.synchronize()
        n = int(d_ntok.item())
        if n != here[0].size or not np.array_equal(d_out[:n].cpu().numpy(), here[0]) or not np.array_equal(d_out_off.cpu().numpy(), here[1]):
            raise AssertionError("leg %s: the ids differ from the parent's" % leg)
    ms = {name: [] for name in runs}
    for r in range(2 + args.repeats):  # two warm-up rounds
        for name, fn in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                fn()
            torch.cuda.synchronize()
            if r >= 2:
                ms[name].append((time.perf_counter() - t0) / args.steps * 1e3)
    parent.swt_bpe_table_destroy(h)
    res = {"ids_equal": True}
    for leg in "cd":
        mine, theirs = ms[leg], ms[leg + "_parent"]
        res[leg] = {"ms_per_step": [round(x, 4) for x in mine], "median": round(statistics.median(mine), 4),
                    "parent_ms_per_step": [round(x, 4) for x in theirs], "parent_median": round(statistics.median(theirs), 4),
                    "parent_spread_ms": round(max(theirs) - min(theirs), 4)}
        res[leg]["passes"] = bool(statistics.median(mine) - statistics.median(theirs) <= max(theirs) - min(theirs))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--leg", choices="abcd", default=None)
    ap.add_argument("--parent-lib", default=None)
    args = ap.parse_args()
    import torch

    from subword_tokenizers_amd import _native as N
    from subword_tokenizers_amd import synth, tokenizers

    N.init(0)
    merges = synth.pretrained_merges()[:8000]
    swapped, where = swap_dependent(merges, 100)
    good, bad = tokenizers.NaiveBPE(), tokenizers.NaiveBPE()
    good.merges_list, bad.merges_list = list(merges), swapped
    tg, tb = good._ensure_naive_table(), bad._ensure_naive_table()
    assert tg.order_equivalent() and not tb.order_equivalent()
    sents = synth.s85k_open()
    text, off = N.pack_utf8([s.lower() for s in sents])
    n_bytes, n_sent = int(text.size), len(sents)
    d_text = torch.from_numpy(np.concatenate([text, np.zeros(64, np.uint8)])).cuda()
    d_off = torch.from_numpy(off.view(np.int64)).cuda()
    d_out = torch.empty(n_bytes + 64, dtype=torch.int32, device="cuda")
    d_out_off = torch.empty(n_sent + 1, dtype=torch.int64, device="cuda")
    d_ntok = torch.zeros(1, dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    legs = {"a": tg.encode_dev, "b": tg.encode_naive_dev, "c": tb.encode_naive_dev, "d": tb.encode_dev}

    def step(leg):
        legs[leg](d_text.data_ptr(), n_bytes, d_off.data_ptr(), n_sent, d_out.data_ptr(), d_out_off.data_ptr(), d_ntok.data_ptr(), 0, stream)

    def result(leg):
        step(leg)
        torch.cuda.synchronize()
        n = int(d_ntok.item())
        return d_out[:n].cpu().numpy().copy(), d_out_off.cpu().numpy().copy()

    if args.leg:
        step(args.leg)
        torch.cuda.synchronize()
        print(json.dumps({"leg": args.leg, "tokens": int(d_ntok.item())}))
        return 0
    out = {"corpus": "S85k-open", "bytes": n_bytes, "sentences": n_sent, "merges": len(merges), "swapped": list(where),
           "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats, "legs": {}}
    ra, rb = result("a"), result("b")
    out["b_equals_a"] = bool(np.array_equal(ra[0], rb[0]) and np.array_equal(ra[1], rb[1]))
    out["tokens"] = {"a": int(ra[0].size), "c": int(result("c")[0].size)}
    for leg in "abcd":
        for _ in range(args.warmup):
            step(leg)
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step(leg)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) / args.steps * 1e3)
        N.profile_enable(True)  # the dominant kernel alone, outside the timed region
        N.profile_read()
        for _ in range(10):
            step(leg)
        torch.cuda.synchronize()
        k_ms, launches = N.profile_read()
        N.profile_enable(False)
        med = statistics.median(ms)
        out["legs"][leg] = {"ms_per_step": [round(x, 4) for x in ms], "median": round(med, 4), "spread": round((max(ms) - min(ms)) / med, 4),
                            "mb_s": round(n_bytes / 1e3 / med, 1), "dominant_kernel_us": round(k_ms * 1e3 / max(launches, 1), 1)}
    a = out["legs"]["a"]["median"]
    out["ratio_to_a"] = {leg: round(out["legs"][leg]["median"] / a, 3) for leg in "bcd"}
    if args.parent_lib:
        out["against_parent"] = against_parent(args, N, torch, bad, step, result, (d_text, n_bytes, d_off, n_sent, d_out, d_out_off, d_ntok, stream))
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
