#!/usr/bin/env python3
"""What swt_mlm_positions_dev and swt_mlm_predict_dev cost next to torch ops that make the same arrays on the device (needs an
MI355X).

Two shapes, each at top_k 1 and 5: FastBPE ids of bench.py's 8,000-merge table, 2,048 rows of S85k-open at width 64, masked at
0.15, with normal logits at V = mask_id() + 1; and FastWP's committed pretrained vocabulary at width 128, with as many rows as
give about the same bytes of logits.  The library leg is what mlm_scores does: the positions, the read-back of their count, the
scores.  The torch leg: logits[labels != -100], logsumexp, topk, and the rank by comparison and sum (the entries equal to the
label's logit at smaller ids counted too, or the ranks would differ wherever two float32 normals tie).  Before the timing both legs
must give the same arrays, the library's lse within lse_tol (tests/fill_cases.py) of torch's float64 logsumexp.  Legs alternate
round after round, HIP events around enough back-to-back calls for 0.2 s.

Without --step this is the driver: every point is a process of its own under its own `timeout`, a failing point ends the run,
and the points' JSON lines go to --out (profiles/fill_mask.txt).  `--step SHAPE:K --library-only` runs the library's calls
alone, for a counter pass around it."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_GBPS = 8000.0  # the data sheet's peak
HBM_COPY_GB_S = 6290.0  # what a float4 copy reaches
ROWS, WIDTH, PROBABILITY = 2048, 64, 0.15
POINTS = [("fastbpe_64", 1), ("fastbpe_64", 5), ("fastwp_128", 1), ("fastwp_128", 5)]
STEP_SECONDS = 240


def torch_leg(torch, logits, labels, k):
    sel = labels != -100
    x = logits[sel]
    lab = labels[sel].long()
    lse = x.logsumexp(1)
    top_v, top_i = x.topk(k, dim=1)
    lv = x.gather(1, lab[:, None])
    ids = torch.arange(x.shape[1], device=x.device)
    rank = (x > lv).sum(1) + ((x == lv) & (ids[None, :] < lab[:, None])).sum(1)
    return lse, top_v, top_i, lv[:, 0], rank


def step(args):
    import torch

    from subword_tokenizers_amd import _native as N
    from subword_tokenizers_amd import synth, tokenizers
    from tests import fill_cases as F

    N.init(0)
    shape, k = args.step.split(":")
    k = int(k)
    if shape == "fastbpe_64":
        tok = tokenizers.FastBPE()
        tok.merges_list = list(synth.pretrained_merges()[:8000])
        tok._build_table()
        rows, width = ROWS, WIDTH
    else:
        tok = tokenizers.FastWP()
        tok.load_resources(os.path.join(ROOT, "tests", "golden", "ref", "resources", "pretrained", "FastWordPiece"))
        bpe = tokenizers.FastBPE()
        bpe.merges_list = list(synth.pretrained_merges()[:8000])
        bpe._build_table()
        width = 128
        rows = max(1, round(ROWS * WIDTH * (bpe.mask_id() + 1) / (width * (tok.mask_id() + 1))))
    V = tok.mask_id() + 1
    texts = synth.s85k_open(85000)[:rows]
    batch = tok.encode_batch(texts, max_length=width, padding="max_length", device=True, mlm={"probability": PROBABILITY, "seed": 7})
    labels = batch["labels"].contiguous()
    gen = torch.Generator(device="cuda").manual_seed(11)
    logits = torch.randn((rows, width, V), device="cuda", generator=gen)
    lib, stream = N.lib(), torch.cuda.current_stream().cuda_stream
    p = lambda a: None if a is None else a.data_ptr()
    cells = rows * width
    d_pos = torch.empty(cells, dtype=torch.int64, device="cuda")
    d_plan, d_info = torch.zeros(2, dtype=torch.int64, device="cuda"), torch.zeros(5, dtype=torch.int64, device="cuda")

    def positions():
        N.check(lib.swt_mlm_positions_dev(p(labels), rows, width, -100, N.FILL_NOT_EQUAL, 0, p(d_pos), p(d_plan), stream))

    positions()
    n = int(d_plan[0])
    types = {np.float32: torch.float32, np.int32: torch.int32}
    out = {name: torch.empty((n, k) if per_k else n, dtype=types[t], device="cuda") for name, t, per_k in N.FILL_OUT}

    def predict():
        N.check(lib.swt_mlm_predict_dev(p(logits), rows, width, V, p(d_pos), n, p(labels), 0, k, *[p(out[name]) for name, _, _ in N.FILL_OUT],
                                        p(d_info), stream))

    def library():
        positions()
        assert int(d_plan.cpu()[0]) == n  # the read-back of mlm_scores
        predict()

    library()
    torch.cuda.synchronize()
    info = d_info.tolist()
    if args.library_only:  # for a counter pass of its own (rocprofv3 --pmc ... -- this step): the library's kernels and no other
        for _ in range(3):
            predict()
        torch.cuda.synchronize()
        print(json.dumps({"shape": shape, "V": V, "top_k": k, "positions": n, "selected_rows_bytes": n * V * 4, "info": info}), flush=True)
        return 0
    # ---- both legs give the same arrays
    lse, top_v, top_i, lv, rank = torch_leg(torch, logits, labels, k)
    assert n == lse.shape[0] and torch.equal(d_pos[:n], (labels != -100).flatten().nonzero()[:, 0])
    x = logits[labels != -100]
    exact = x.double().logsumexp(1)
    err = (out["lse"].double() - exact).abs()
    tol = torch.tensor([F.lse_tol(V, N.fill_capacity()[0], float(v)) for v in exact.cpu()], dtype=torch.float64, device="cuda")
    assert bool((err <= tol).all()), "lse: %.3f x 2^-24 off" % float((err / tol).max())
    assert torch.allclose(out["lse"], lse, rtol=0, atol=float(tol.max()) + V * F.U * float(exact.abs().max().clamp(min=1.0)))
    assert torch.equal(out["top_logit"], top_v) and torch.equal(x.gather(1, out["top_id"].long()), top_v)
    distinct = (top_v[:, 1:] != top_v[:, :-1]).all(1) if k > 1 else torch.ones(n, dtype=torch.bool, device="cuda")
    assert torch.equal(out["top_id"][distinct].long(), top_i[distinct])
    assert torch.equal(out["label_logit"], lv) and torch.equal(out["label_rank"].long(), rank) and torch.equal(out["label_id"].long(), labels[labels != -100].long())
    assert info[0] == n and info[1] == int((rank == 0).sum()) and info[2] == int((rank < k).sum()) and info[3] == 0 and info[4] == 0
    worst = float((err / F.U).max())
    del x, exact, err, tol, lse, top_v, top_i, lv, rank

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record(); e1.synchronize()
        return e0.elapsed_time(e1) / reps

    legs = {"library": library, "torch": lambda: torch_leg(torch, logits, labels, k), "mlm_positions_dev": positions, "mlm_predict_dev": predict}
    reps = {name: max(1, int(np.ceil(200.0 / max(timed(fn, 3), 1e-3)))) for name, fn in legs.items()}
    ms = {name: [] for name in legs}
    for r in range(args.warmup + args.rounds):
        t = {name: timed(fn, reps[name]) for name, fn in legs.items()}  # the legs alternate inside a round
        if r >= args.warmup:
            for name, v in t.items():
                ms[name].append(v)
    res = {name: {"ms": [round(x, 4) for x in v], "median_ms": round(statistics.median(v), 4),
                  "spread": round((max(v) - min(v)) / statistics.median(v), 4)} for name, v in ms.items()}
    nbytes = n * V * 4
    for name in ("library", "mlm_predict_dev"):
        gbps = nbytes / res[name]["median_ms"] / 1e6
        res[name].update({"rows_gb_s": round(gbps, 1), "share_of_hbm_peak": round(gbps / HBM_GBPS, 4), "share_of_hbm_copy": round(gbps / HBM_COPY_GB_S, 4)})
    res["torch"]["ratio_to_library"] = round(res["torch"]["median_ms"] / res["library"]["median_ms"], 2)
    line = json.dumps({"shape": shape, "rows": rows, "width": width, "V": V, "top_k": k, "positions": n, "selected_rows_bytes": nbytes,
                       "logits_bytes": cells * V * 4, "info": info, "lse_largest_error_in_2^-24": round(worst, 3),
                       "lse_tol_in_2^-24_at_lse_0": round(F.lse_tol(V, N.fill_capacity()[0]) / F.U, 1), "rounds": args.rounds,
                       "calls_per_window": reps, "legs": res})
    print(line, flush=True)
    if args.out:
        with open(args.out, "a", encoding="utf-8") as f:
            f.write(line + "\n")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--step", default=None, help="SHAPE:TOP_K, one point in this process")
    ap.add_argument("--library-only", action="store_true", help="with --step: the library's calls a few times and nothing else")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fill_mask.txt"))
    args = ap.parse_args()
    if args.step:
        return step(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").close()
    for shape, k in POINTS:  # a process and a time limit per point; the first that fails ends the run
        cmd = ["timeout", "-k", "10", str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), "--step", "%s:%d" % (shape, k),
               "--rounds", str(args.rounds), "--warmup", str(args.warmup), "--out", args.out]
        rc = subprocess.run(cmd, cwd=ROOT).returncode
        if rc:
            print("gpu_fill: %s top_k %d ended with status %d; nothing more is started" % (shape, k, rc), file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
