#!/usr/bin/env python3
"""What the device normalizer costs (needs an MI355X).  S85k-open, every point a process of its own:

  kernels   swt_normalize_plan_dev, swt_normalize_rows_dev with and without SWT_NORMALIZE_ALIGN (all four flags) and
            swt_utf8_lower_dev over the same resident text, a few calls each under `rocprofv3 --kernel-trace --stats`, a run of its
            own: the device time of every kernel, the GB/s of source text, and the share of the HBM peak of the traffic the design
            implies (source read once from memory, output written once, 4 bytes per code point of alignment)
  counters  the same calls under `rocprofv3 --pmc FETCH_SIZE` and nothing else (the counter takes three of the four slots of a run): what each kernel fetched from memory --
            whether the rows' second read of a tile is served by L2
  encode    encode_batch(texts, max_length=64, device=True) through FastBPE: the wall clock with no normalizer in this tree and,
            with --parent DIR (a built checkout of the parent commit), in that tree, alternating; with "bert" in this tree; and the
            device time of a plain call of both trees from kernel traces of their own

The JSON lines go to --out (profiles/normalizer.txt).  A failing point ends the run."""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_GBPS = 8000.0  # the data sheet's peak
STEP_SECONDS = 200
TRACE_CALLS = 4


def emit(args, rec):
    print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, "a", encoding="utf-8") as f:
            f.write(json.dumps(rec) + "\n")
    return 0


def step(args):
    sys.path.insert(0, os.path.abspath(args.root or ROOT))
    import numpy as np
    import torch

    from subword_tokenizers_amd import _native as N
    from subword_tokenizers_amd import synth, tokenizers

    N.init(0)
    texts = synth.s85k_open(85000)
    if args.step == "encode":
        tok = tokenizers.FastBPE()
        tok.merges_list = list(synth.pretrained_merges()[:8000])
        tok._build_table()
        if args.normalizer:
            tok.set_normalizer(args.normalizer)
        rec = {"point": "encode:" + (args.normalizer or "plain"), "root": "parent" if args.root else "this"}

        def call():
            tok.encode_batch(texts, max_length=64, device=True)
            torch.cuda.synchronize()

        call()
        if args.trace:
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
        return emit(args, rec)

    # the four device calls over the resident text, TRACE_CALLS times each, for a trace or a counter run around them
    from subword_tokenizers_amd import batching
    text, off = N.pack_utf8(texts)
    n, n_sent, lib, stream = int(text.size), len(texts), N.lib(), torch.cuda.current_stream().cuda_stream
    d_text = torch.from_numpy(np.concatenate([text, np.zeros(64, dtype=np.uint8)])).cuda()
    d_off = torch.from_numpy(off.view(np.int64)).cuda()
    flags = batching.normalizer_flags(batching.normalizer_setting("bert"))
    d_info = torch.zeros(3, dtype=torch.int64, device="cuda")
    plan = lambda: N.check(lib.swt_normalize_plan_dev(d_text.data_ptr(), n, d_off.data_ptr(), n_sent, flags, d_info.data_ptr(), stream))
    plan()
    out_bytes, out_cps, src_cps = (int(x) for x in d_info.cpu())
    d_out = torch.empty(out_bytes + 64, dtype=torch.uint8, device="cuda")
    d_o = [torch.empty(n_sent + 1, dtype=torch.int64, device="cuda") for _ in range(3)]
    d_align, d_flag = torch.empty(out_cps + 1, dtype=torch.int32, device="cuda"), torch.empty(n_sent + 16, dtype=torch.uint8, device="cuda")
    d_copy = d_text.clone()
    rows = lambda f, a: N.check(lib.swt_normalize_rows_dev(d_text.data_ptr(), n, d_off.data_ptr(), n_sent, flags | f, d_out.data_ptr(), out_bytes,
                                                          d_o[0].data_ptr(), *a, stream))
    for _ in range(TRACE_CALLS):
        plan()
        rows(0, (None, None, None, 0))
        rows(N.NORMALIZE_ALIGN, (d_o[1].data_ptr(), d_o[2].data_ptr(), d_align.data_ptr(), out_cps))
        N.check(lib.swt_utf8_lower_dev(d_copy.data_ptr(), n, d_off.data_ptr(), n_sent, d_flag.data_ptr(), stream))
    torch.cuda.synchronize()
    print(json.dumps({"point": "text", "texts": n_sent, "source_bytes": n, "normalised_bytes": out_bytes, "normalised_cps": out_cps,
                      "source_cps": src_cps}), flush=True)
    return 0


def profiled(me, tool_args, child_args, pattern):
    """the child under rocprofv3 with tool_args -> (what the child printed, the rows of the csv files that match pattern)"""
    out_dir = tempfile.mkdtemp(prefix="normalize_prof_")
    cmd = ["timeout", "-k", "10", str(STEP_SECONDS), "rocprofv3"] + tool_args + ["--output-format", "csv", "-d", out_dir, "--", sys.executable, me,
                                                                               "--out", ""] + child_args
    run = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, text=True)
    if run.returncode:
        return run.returncode, None, None
    told = json.loads([line for line in run.stdout.splitlines() if line.startswith("{")][-1])
    rows = []
    for path in glob.glob(os.path.join(out_dir, "**", pattern), recursive=True):
        with open(path, newline="") as f:
            rows.extend(csv.DictReader(f))
    return 0, told, rows


def short(name):
    return name.split("(")[0].replace("void ", "")


def kernels(args, me):
    rc, told, rows = profiled(me, ["--kernel-trace", "--stats"], ["--step", "device"], "*kernel_stats.csv")
    if rc:
        return rc
    emit(args, told)
    n, out, cps = told["source_bytes"], told["normalised_bytes"], told["normalised_cps"]
    implied = {"swt::norm_kernel<false, false>": n, "swt::norm_kernel<true, false>": n + out, "swt::norm_kernel<true, true>": n + out + 4 * cps,
               "swt::lower_kernel": 2 * n}
    for row in rows:
        name = short(row["Name"])
        if "swt::" not in name:
            continue
        us = float(row["AverageNs"]) / 1e3
        rec = {"point": "kernel", "kernel": name, "calls": int(row["Calls"]), "average_us": round(us, 2)}
        if name in implied:
            rec.update({"source_gb_s": round(n / us / 1e3, 1), "implied_traffic_bytes": implied[name],
                        "implied_share_of_hbm_peak": round(implied[name] / us / 1e3 / HBM_GBPS, 4)})
        emit(args, rec)
    return 0


def counters(args, me):
    rc, told, rows = profiled(me, ["--pmc", "FETCH_SIZE"], ["--step", "device"], "*counter_collection.csv")
    if rc:
        return rc
    acc = {}
    for row in rows:
        name = short(row["Kernel_Name"])
        if "swt::norm_kernel" in name or "swt::lower_kernel" in name:
            acc.setdefault(name, {}).setdefault(row["Counter_Name"], []).append(float(row["Counter_Value"]))
    for name, c in sorted(acc.items()):
        emit(args, {"point": "counters", "kernel": name, "source_bytes": told["source_bytes"], "normalised_bytes": told["normalised_bytes"],
                    **{k + "_mean": round(statistics.mean(v), 1) for k, v in c.items()}, "dispatches": len(next(iter(c.values())))})
    return 0 if acc else 1


def encode_device(args, me, root):
    rc, told, rows = profiled(me, ["--kernel-trace", "--stats"], ["--step", "encode", "--trace"] + (["--root", root] if root else []),
                              "*kernel_stats.csv")
    if rc:
        return rc
    swt = {short(r["Name"]): float(r["TotalDurationNs"]) for r in rows if "swt::" in r["Name"]}
    return emit(args, {"point": "encode:plain:device", "root": told["root"], "calls": TRACE_CALLS,
                       "library_kernels_us_per_call": round(sum(swt.values()) / 1e3 / TRACE_CALLS, 1), "library_kernels": len(swt),
                       "normalizer_kernels": sorted(k for k in swt if "norm_" in k)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step", default=None, help="device or encode: one point in this process")
    ap.add_argument("--trace", action="store_true", help="with --step encode: a few calls and no timing, for a trace around them")
    ap.add_argument("--normalizer", default=None, help="with --step encode: the set_normalizer argument")
    ap.add_argument("--root", default=None, help="with --step encode: the tree whose package is measured")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normalizer.txt"))
    args = ap.parse_args()
    if args.step:
        return step(args)
    me = os.path.abspath(__file__)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").close()
    if (rc := kernels(args, me)):
        return rc
    if (rc := counters(args, me)):
        return rc
    base = ["timeout", "-k", "10", str(STEP_SECONDS), sys.executable, me, "--rounds", str(args.rounds), "--warmup", str(args.warmup), "--out", args.out,
            "--step", "encode"]
    legs = [[]] + ([["--root", args.parent]] if args.parent else [])
    for extra in legs + legs + [["--normalizer", "bert"]]:  # the plain legs twice, alternating; a process and a time limit per point
        rc = subprocess.run(base + extra, cwd=ROOT).returncode
        if rc:
            print("gpu_normalize: %s ended with status %d; nothing more is started" % (" ".join(extra), rc), file=sys.stderr)
            return rc
    for root in [None] + ([args.parent] if args.parent else []):
        if (rc := encode_device(args, me, root)):
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
