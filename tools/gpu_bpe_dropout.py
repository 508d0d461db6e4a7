#!/usr/bin/env python3
"""What BPE-dropout costs next to the plain FastBPE encode, and that the plain encode did not move (needs an MI355X; DESIGN.md
4.2e).

S85k-open, bench.py's 8,000-merge table, the lowercased text resident on the device.  Legs that alternate round after round in
one process, HIP events around enough back-to-back calls for 0.2 s each:
  plain            swt_bpe_encode_dev with SWT_OPT_DEDUP = 1 (every occurrence encoded: the lane kernel alone), this tree
  plain_parent     the same call into the parent commit's library (--parent-lib, a second libswt_hip.so loaded beside this
                   tree's), when one is given: the number that must not move, held to the spread measured in this same run
  dropout_draws    swt_bpe_encode_dropout_dev at drop_below = 1: every draw made, effectively none dropped
  dropout_p10      the same at p = 0.1
  dropout_draws_parent, dropout_p10_parent   the two dropout legs through the parent's library (--parent-lib), their ids compared
                   with this tree's first.  "dropout_against_parent": a leg passes when this tree's median does not exceed the
                   parent's by more than the parent's own spread (max - min) in this run
Before the timing the dropout ids at drop_below = 0 are compared with the plain ids on the whole text, and those at p = 0.1
with the model of tests/dropout_cases.py on the first --check sentences.  Prints one JSON line; --out FILE appends it."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED, EPOCH = 2024, 0
NEEDED = ("swt_init", "swt_last_error", "swt_bpe_table_create", "swt_bpe_table_destroy", "swt_bpe_table_set_option", "swt_bpe_encode_dev",
          "swt_bpe_encode_dropout_dev")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sentences", type=int, default=85000)
    ap.add_argument("--check", type=int, default=300)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from subword_tokenizers_amd import _native as N
    from subword_tokenizers_amd import synth, tokenizers
    from tests import dropout_cases as D

    N.init(0)
    merges = [tuple(m) for m in synth.pretrained_merges()[:8000]]
    syms = tokenizers._SymbolTable()
    tri = np.array([x for l, r in merges for x in (syms.intern(l), syms.intern(r), syms.intern(l + r))], dtype=np.uint32).reshape(-1, 3)
    left, right, merged = (np.ascontiguousarray(tri[:, k]) for k in range(3))
    sents = synth.s85k_open(args.sentences)
    text, off = N.pack_and_lower(sents)
    n_bytes, n_sent = int(text.size), len(sents)
    stream = torch.cuda.current_stream().cuda_stream
    d_text = torch.from_numpy(np.concatenate([text, np.zeros(64, dtype=np.uint8)])).cuda()
    d_off = torch.from_numpy(off.view(np.int64)).cuda()
    d_ids, d_ids2 = (torch.zeros(n_bytes + 64, dtype=torch.int32, device="cuda") for _ in range(2))
    d_tok_off, d_ntok = torch.zeros(n_sent + 1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")

    def table(lib):
        h = C.c_void_p()
        rc = lib.swt_bpe_table_create(N.ptr(left, N.u32p), N.ptr(right, N.u32p), N.ptr(merged, N.u32p), len(merges), C.byref(h))
        rc = rc or lib.swt_bpe_table_set_option(h, N.OPT_DEDUP, N.DEDUP_NEVER)
        if rc:
            raise RuntimeError("table: %d %s" % (rc, lib.swt_last_error().decode()))
        return h

    def plain_of(lib, h, out=d_ids):
        def call():
            rc = lib.swt_bpe_encode_dev(h, d_text.data_ptr(), n_bytes, d_off.data_ptr(), n_sent, out.data_ptr(), d_tok_off.data_ptr(),
                                        d_ntok.data_ptr(), 0, stream)
            if rc:
                raise RuntimeError("swt_bpe_encode_dev: %d %s" % (rc, lib.swt_last_error().decode()))
        return call

    here = N.lib()
    h_here = table(here)
    legs = {"plain": plain_of(here, h_here)}
    if args.parent_lib:
        parent = C.CDLL(os.path.abspath(args.parent_lib))
        for name in NEEDED:
            fn = getattr(parent, name)
            fn.restype, fn.argtypes = N.SIGNATURES[name]
        if parent.swt_init(0):
            raise RuntimeError("the parent's library does not initialise")
        h_parent = table(parent)
        legs["plain_parent"] = plain_of(parent, h_parent)

    def dropout_of(below, out=d_ids, n=n_sent, nb=n_bytes, lib=here, h=h_here):
        def call():
            rc = lib.swt_bpe_encode_dropout_dev(h, d_text.data_ptr(), nb, d_off.data_ptr(), n, out.data_ptr(), d_tok_off.data_ptr(),
                                                d_ntok.data_ptr(), 0, below, SEED, EPOCH, stream)
            if rc:
                raise RuntimeError("swt_bpe_encode_dropout_dev: %d %s" % (rc, lib.swt_last_error().decode()))
        return call

    drops = {"dropout_draws": 1, "dropout_p10": D.drop_below(0.1)}
    for name, below in drops.items():
        legs[name] = dropout_of(below)
        if "plain_parent" in legs:
            legs[name + "_parent"] = dropout_of(below, lib=parent, h=h_parent)

    # ---- the checks
    legs["plain"]()
    torch.cuda.synchronize()
    n_plain = int(d_ntok.item())
    dropout_of(0, d_ids2)()
    torch.cuda.synchronize()
    if int(d_ntok.item()) != n_plain or not torch.equal(d_ids[:n_plain], d_ids2[:n_plain]):
        raise AssertionError("drop_below = 0 differs from swt_bpe_encode_dev")
    if "plain_parent" in legs:
        plain_of(parent, h_parent, d_ids2)()
        torch.cuda.synchronize()
        if int(d_ntok.item()) != n_plain or not torch.equal(d_ids[:n_plain], d_ids2[:n_plain]):
            raise AssertionError("the plain encode differs from the parent's")
    tokens = {}
    for name, below in drops.items():
        legs[name]()
        torch.cuda.synchronize()
        tokens[name] = int(d_ntok.item())
        if "plain_parent" in legs:
            dropout_of(below, d_ids2, lib=parent, h=h_parent)()
            torch.cuda.synchronize()
            if int(d_ntok.item()) != tokens[name] or not torch.equal(d_ids[:tokens[name]], d_ids2[:tokens[name]]):
                raise AssertionError("%s differs from the parent's" % name)
    k = min(args.check, n_sent)
    d_off_k = d_off[:k + 1].clone()  # the first k sentences as a call of their own: same indices, same bytes, same ids
    N.check(here.swt_bpe_encode_dropout_dev(h_here, d_text.data_ptr(), int(off[k]), d_off_k.data_ptr(), k, d_ids2.data_ptr(), d_tok_off.data_ptr(),
                                            d_ntok.data_ptr(), 0, D.drop_below(0.1), SEED, EPOCH, stream))
    torch.cuda.synchronize()
    want = D.ids_of(D.tokenize(D.Table(merges), tokenizers.SubwordTokenizer._split, sents[:k], D.drop_below(0.1), SEED, EPOCH),
                    lambda s: N.SYM_BASE + syms.index[s])
    got = d_ids2[:int(d_ntok.item())].cpu().numpy().view(np.uint32)
    if not np.array_equal(got, want[0]) or not np.array_equal(d_tok_off[:k + 1].cpu().numpy().view(np.uint64), want[1]):
        raise AssertionError("p = 0.1 differs from the model on the first %d sentences" % k)

    # ---- the timing
    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record(); e1.synchronize()
        return e0.elapsed_time(e1) / reps

    reps = {name: max(1, int(np.ceil(200.0 / max(timed(fn, 10), 1e-3)))) for name, fn in legs.items()}
    ms = {name: [] for name in legs}
    for r in range(args.warmup + args.rounds):
        t = {name: timed(fn, reps[name]) for name, fn in legs.items()}
        if r >= args.warmup:
            for name, v in t.items():
                ms[name].append(v)
    out = {"corpus": "S85k-open", "sentences": n_sent, "bytes": n_bytes, "merges": len(merges), "tokens_plain": n_plain, "tokens": tokens,
           "checked_against_model": k, "rounds": args.rounds, "calls_per_window": reps, "legs": {}}
    for name, v in ms.items():
        med = statistics.median(v)
        out["legs"][name] = {"ms": [round(x, 4) for x in v], "median_ms": round(med, 4), "spread": round((max(v) - min(v)) / med, 4)}
    base = out["legs"]["plain"]["median_ms"]
    for name in ("dropout_draws", "dropout_p10"):
        out["legs"][name]["ratio_to_plain"] = round(out["legs"][name]["median_ms"] / base, 2)
    if "plain_parent" in legs:
        p = out["legs"]["plain_parent"]
        out["plain_against_parent"] = {"ratio": round(base / p["median_ms"], 4),
                                       "margin": round(max(p["spread"], out["legs"]["plain"]["spread"]), 4)}
        out["dropout_against_parent"] = {}
        for name in drops:
            theirs = ms[name + "_parent"]
            over = statistics.median(ms[name]) - statistics.median(theirs)
            out["dropout_against_parent"][name] = {"over_parent_ms": round(over, 4), "parent_spread_ms": round(max(theirs) - min(theirs), 4),
                                                   "passes": bool(over <= max(theirs) - min(theirs))}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a", encoding="utf-8") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
