#!/usr/bin/env python3
"""What added tokens cost in encode_batch (needs an MI355X).

S85k-open through FastBPE over bench.py's 8,000-merge table, encode_batch(..., max_length=64, padding="max_length", device=True),
the wall clock of a call with the device drained, every point a process of its own:

  plain       no added token registered -- in this tree and, with --parent DIR (a built checkout of the parent commit), in that
              tree, the two alternating round after round in the same run; the launches are the same, so the two are expected to
              agree within the spread the file records beside them
  registered  add_special_tokens(["[MASK]"]) and the same texts, which hold none: the cost of swt_added_find, of the span form the
              encode then takes, and of swt_added_splice
  masked      the same texts with "[MASK]" written over 15 % of the words (seed 15), and beside it Python's `re` finding the same
              matches in the lowercased host strings
  long        swt_added_find_dev alone over the first MiB of `masked`: as ONE text, which one wavefront walks from end to end, and
              as the texts it is made of
  kernels     `plain`, `registered` and `masked` a few times each under `rocprofv3 --kernel-trace --stats`, runs of their own: the
              device time of a call -- the wall clock above is mostly host work --, the library's kernels, and the find kernel's
              text bytes per second beside the HBM peak the other profiles quote

The points' JSON lines go to --out (profiles/added_tokens.txt).  A failing point ends the run."""
import argparse
import csv
import glob
import json
import os
import random
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_GBPS = 8000.0  # the data sheet's peak
WIDTH, SHARE, SEED = 64, 0.15, 15
STEP_SECONDS = 280
TRACE_CALLS = 4


def masked(texts):
    rng, out = random.Random(SEED), []
    for t in texts:
        words = t.split(" ")
        out.append(" ".join("[MASK]" if w and rng.random() < SHARE else w for w in words))
    return out


def step(args):
    root = os.path.abspath(args.root or ROOT)
    sys.path.insert(0, root)
    import torch

    from subword_tokenizers_amd import _native as N
    from subword_tokenizers_amd import synth, tokenizers

    N.init(0)
    tok = tokenizers.FastBPE()
    tok.merges_list = list(synth.pretrained_merges()[:8000])
    tok._build_table()
    texts = synth.s85k_open(85000)
    n_bytes = sum(len(t.lower().encode("utf-8")) for t in texts)
    rec = {"point": args.step, "root": "parent" if args.root else "this", "texts": len(texts)}
    if args.step in ("registered", "masked", "long"):
        tok.add_special_tokens(["[MASK]"])
    if args.step in ("masked", "long"):
        texts = masked(texts)
        n_bytes = sum(len(t.lower().encode("utf-8")) for t in texts)
    rec["text_bytes"] = n_bytes

    if args.step == "long":  # swt_added_find_dev alone: a MiB of text as one text (one wavefront walks it) and as the texts it came from
        import numpy as np
        text, off = N.pack_utf8([t.lower() for t in texts])
        n_sent = int(np.searchsorted(off, 1 << 20))
        n = int(off[n_sent])
        d_text = torch.from_numpy(np.concatenate([text[:n], np.zeros(64, dtype=np.uint8)])).cuda()
        d_out, d_pat, d_span = torch.empty_like(d_text), torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(2 * n, dtype=torch.int32, device="cuda")
        d_info, stream, handle = torch.zeros(4, dtype=torch.int64, device="cuda"), torch.cuda.current_stream().cuda_stream, tok._added_patterns()
        for name, offsets in (("as_one_text", np.array([0, n], dtype=np.uint64)), ("as_texts", off[:n_sent + 1])):
            d_off = torch.from_numpy(offsets.view(np.int64).copy()).cuda()
            d_m_off = torch.empty(offsets.size, dtype=torch.int64, device="cuda")
            ms = []
            for r in range(args.warmup + args.rounds):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                handle.find_dev(d_text.data_ptr(), n, d_off.data_ptr(), offsets.size - 1, d_out.data_ptr(), d_m_off.data_ptr(), d_pat.data_ptr(),
                                d_span.data_ptr(), d_info.data_ptr(), stream)
                e1.record(); e1.synchronize()
                if r >= args.warmup:
                    ms.append(e0.elapsed_time(e1))
            rec[name] = {"texts": int(offsets.size - 1), "bytes": n, "find_ms": [round(x, 4) for x in ms], "median_ms": round(statistics.median(ms), 4),
                         "matches": int(d_info[0])}
        return emit(args, rec)

    def call():
        out = tok.encode_batch(texts, max_length=WIDTH, padding="max_length", device=True)
        torch.cuda.synchronize()
        return out

    out = call()
    if args.step != "plain":
        rec["mask_columns"] = int((out["input_ids"] == tok.mask_id()).sum())
    if args.trace:  # under rocprofv3: TRACE_CALLS calls and nothing else
        for _ in range(TRACE_CALLS - 1):
            call()
        print(json.dumps(rec), flush=True)
        return 0
    ms = []
    for r in range(args.warmup + args.rounds):
        t0 = time.perf_counter()
        call()
        if r >= args.warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    rec.update({"ms": [round(x, 2) for x in ms], "median_ms": round(statistics.median(ms), 2),
                "spread": round((max(ms) - min(ms)) / statistics.median(ms), 4)})
    if args.step == "masked":  # for orientation: the same matches from `re` over the host strings
        low = [t.lower() for t in texts]
        pat = re.compile(re.escape("[mask]"))
        t0 = time.perf_counter()
        n = sum(1 for t in low for _ in pat.finditer(t))
        rec["re_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
        rec["re_matches"] = n
        rec["matches_in_rows"] = rec["mask_columns"]  # fewer where a row of 64 columns cuts its text short
    return emit(args, rec)


def emit(args, rec):
    print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, "a", encoding="utf-8") as f:
            f.write(json.dumps(rec) + "\n")
    return 0


def kernels(args, me):
    """`plain`, `registered` and `masked` under rocprofv3, a run each: per point one JSON line with the library's kernels (calls,
    average us), the device time of a call (every kernel's total over the calls) and, where the find kernel runs, its text bytes
    per second.  A point whose stats lack the find kernel where it must run is a failure."""
    for point in ("plain", "registered", "masked"):
        out_dir = tempfile.mkdtemp(prefix="added_tokens_trace_")
        cmd = ["timeout", "-k", "10", str(STEP_SECONDS), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir, "--",
               sys.executable, me, "--step", point, "--trace", "--out", ""]
        run = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, text=True)
        if run.returncode:
            return run.returncode
        told = json.loads([line for line in run.stdout.splitlines() if line.startswith("{")][-1])
        rows, total_ns = {}, 0.0
        for path in glob.glob(os.path.join(out_dir, "**", "*kernel_stats.csv"), recursive=True):
            with open(path, newline="") as f:
                for row in csv.DictReader(f):
                    total_ns += float(row["TotalDurationNs"])
                    if "swt::" in row["Name"]:
                        rows[row["Name"].split("(")[0].replace("void ", "")] ={"calls": int(row["Calls"]), "average_us": round(float(row["AverageNs"]) / 1e3, 2)}
        rec = {"point": "kernels:" + point, "text_bytes": told["text_bytes"], "calls": TRACE_CALLS,
               "device_us_per_call": round(total_ns / 1e3 / TRACE_CALLS, 1), "kernels": rows}
        find = rows.get("swt::added_find_kernel")
        if point != "plain":
            if not find or find["calls"] != TRACE_CALLS:
                print("gpu_added_tokens: the stats of %s hold no swt::added_find_kernel for every call: %s" % (point, sorted(rows)), file=sys.stderr)
                return 1
            gbps = told["text_bytes"] / find["average_us"] / 1e3
            rec["find_text_gb_s"], rec["find_share_of_hbm_peak"] = round(gbps, 1), round(gbps / HBM_GBPS, 4)
        elif find:
            print("gpu_added_tokens: swt::added_find_kernel ran with no added token registered", file=sys.stderr)
            return 1
        emit(args, rec)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--step", default=None, help="plain, registered, masked or long: one point in this process")
    ap.add_argument("--trace", action="store_true", help="with --step: the point's call a few times and no timing, for a trace around it")
    ap.add_argument("--root", default=None, help="with --step plain: the tree whose package is measured (a checkout of the parent commit)")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit, for the second `plain` leg")
    ap.add_argument("--kernels-only", action="store_true", help="the `kernels` points alone, appended to --out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "added_tokens.txt"))
    args = ap.parse_args()
    if args.step:
        return step(args)
    me = os.path.abspath(__file__)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if args.kernels_only:
        return kernels(args, me)
    open(args.out, "w").close()
    base = ["timeout", "-k", "10", str(STEP_SECONDS), sys.executable, me, "--rounds", str(args.rounds), "--warmup", str(args.warmup), "--out", args.out]
    legs = [["--step", "plain"]] + ([["--step", "plain", "--root", args.parent]] if args.parent else [])
    points = legs + legs + [["--step", "registered"], ["--step", "masked"], ["--step", "long"]]  # the plain legs twice, alternating
    for extra in points:  # a process and a time limit per point; the first that fails ends the run
        rc = subprocess.run(base + extra, cwd=ROOT).returncode
        if rc:
            print("gpu_added_tokens: %s ended with status %d; nothing more is started" % (" ".join(extra), rc), file=sys.stderr)
            return rc
    return kernels(args, me)


if __name__ == "__main__":
    sys.exit(main())
