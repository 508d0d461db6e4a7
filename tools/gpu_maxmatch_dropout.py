#!/usr/bin/env python3
"""What MaxMatch-Dropout costs next to the plain NaiveWP encode, and that the plain encode did not move (needs an MI355X;
DESIGN.md 4.3d).

S85k, the pretrained 20,000-token vocabulary, the lowercased text resident on the device.  Legs that alternate round after round
in one process, HIP events around enough back-to-back calls for 0.2 s each:
  plain            swt_wp_encode_naive_dev, this tree
  plain_parent     the same call into the parent commit's library (--parent-lib, a second libswt_hip.so loaded beside this
                   tree's), when one is given: the number that must not move, held to the spread measured in this same run
  dropout_draws    swt_wp_encode_naive_dropout_dev at drop_below = 1: every draw made, effectively none dropped
  dropout_p10      the same at p = 0.1
  dropout_draws@X  dropout_draws through another build of the library (--variant-lib X=PATH, repeatable): scratch builds that
                   leave a part of the work out, to say where the time goes
Before the timing the dropout ids at drop_below = 0 are compared with the plain ids on the whole text, and those at p = 0.1
with the model of tests/maxmatch_cases.py on the first --check sentences.  Prints one JSON line; --out FILE appends it."""
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
NEEDED = ("swt_init", "swt_last_error", "swt_wp_trie_create", "swt_wp_trie_destroy", "swt_wp_encode_naive_dev")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sentences", type=int, default=85000)
    ap.add_argument("--check", type=int, default=300)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--variant-lib", action="append", default=[], metavar="NAME=PATH")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from subword_tokenizers_amd import _native as N
    from subword_tokenizers_amd import synth, tokenizers
    from tests import maxmatch_cases as M

    N.init(0)
    vocab = sorted(set(synth.pretrained_vocab()))
    blob, voff = N.pack_utf32(vocab)
    sents = synth.s85k()[:args.sentences]
    text, off = N.pack_and_lower(sents)
    n_bytes, n_sent = int(text.size), len(sents)
    stream = torch.cuda.current_stream().cuda_stream
    d_text = torch.from_numpy(np.concatenate([text, np.zeros(64, dtype=np.uint8)])).cuda()
    d_off = torch.from_numpy(off.view(np.int64)).cuda()
    d_ids, d_ids2 = (torch.zeros(n_bytes + 64, dtype=torch.int32, device="cuda") for _ in range(2))
    d_tok_off, d_ntok = torch.zeros(n_sent + 1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
    d_status, d_status2 = (torch.zeros(n_sent + 8, dtype=torch.uint8, device="cuda") for _ in range(2))

    def trie(lib):
        h = C.c_void_p()
        if lib.swt_wp_trie_create(N.ptr(blob, N.u32p), N.ptr(voff, N.u64p), len(vocab), C.byref(h)):
            raise RuntimeError("trie: %s" % lib.swt_last_error().decode())
        return h

    def plain_of(lib, h, out=d_ids, st=d_status):
        def call():
            rc = lib.swt_wp_encode_naive_dev(h, d_text.data_ptr(), n_bytes, d_off.data_ptr(), n_sent, out.data_ptr(), d_tok_off.data_ptr(),
                                             st.data_ptr(), d_ntok.data_ptr(), stream)
            if rc:
                raise RuntimeError("swt_wp_encode_naive_dev: %d %s" % (rc, lib.swt_last_error().decode()))
        return call

    here = N.lib()
    h_here = trie(here)
    legs = {"plain": plain_of(here, h_here)}
    if args.parent_lib:
        parent = C.CDLL(os.path.abspath(args.parent_lib))
        for name in NEEDED:
            fn = getattr(parent, name)
            fn.restype, fn.argtypes = N.SIGNATURES[name]
        if parent.swt_init(0):
            raise RuntimeError("the parent's library does not initialise")
        h_parent = trie(parent)
        legs["plain_parent"] = plain_of(parent, h_parent)

    def dropout_of(below, out=d_ids, st=d_status, lib=here, h=h_here):
        def call():
            if lib.swt_wp_encode_naive_dropout_dev(h, d_text.data_ptr(), n_bytes, d_off.data_ptr(), n_sent, out.data_ptr(), d_tok_off.data_ptr(),
                                                   st.data_ptr(), d_ntok.data_ptr(), below, SEED, EPOCH, stream):
                raise RuntimeError("swt_wp_encode_naive_dropout_dev: %s" % lib.swt_last_error().decode())
        return call

    legs["dropout_draws"] = dropout_of(1)
    legs["dropout_p10"] = dropout_of(M.drop_below(0.1))
    for spec in args.variant_lib:
        name, _, path = spec.partition("=")
        var = C.CDLL(os.path.abspath(path))
        for fn_name in NEEDED + ("swt_wp_encode_naive_dropout_dev",):
            fn = getattr(var, fn_name)
            fn.restype, fn.argtypes = N.SIGNATURES[fn_name]
        if var.swt_init(0):
            raise RuntimeError("the library of %s does not initialise" % name)
        legs["dropout_draws@" + name] = dropout_of(1, lib=var, h=trie(var))

    # ---- the checks
    def same_as_plain(what):
        torch.cuda.synchronize()
        if int(d_ntok.item()) != n_plain or not torch.equal(d_ids[:n_plain], d_ids2[:n_plain]) or not torch.equal(d_status[:n_sent], d_status2[:n_sent]):
            raise AssertionError(what)

    legs["plain"]()
    torch.cuda.synchronize()
    n_plain = int(d_ntok.item())
    dropout_of(0, d_ids2, d_status2)()
    same_as_plain("drop_below = 0 differs from swt_wp_encode_naive_dev")
    if "plain_parent" in legs:
        plain_of(parent, h_parent, d_ids2, d_status2)()
        same_as_plain("the plain encode differs from the parent's")
    tokens, refused = {}, {}
    for name in ("dropout_draws", "dropout_p10"):
        legs[name]()
        torch.cuda.synchronize()
        tokens[name], refused[name] = int(d_ntok.item()), int((d_status[:n_sent] != 0).sum().item())
    k = min(args.check, n_sent)
    d_off_k = d_off[:k + 1].clone()  # the first k sentences as a call of their own: same indices, same bytes, same ids
    N.check(here.swt_wp_encode_naive_dropout_dev(h_here, d_text.data_ptr(), int(off[k]), d_off_k.data_ptr(), k, d_ids2.data_ptr(),
                                                 d_tok_off.data_ptr(), d_status2.data_ptr(), d_ntok.data_ptr(), M.drop_below(0.1), SEED, EPOCH,
                                                 stream))
    torch.cuda.synchronize()
    want = M.Model(vocab).batch(tokenizers.SubwordTokenizer._split, sents[:k], M.drop_below(0.1), SEED, EPOCH)
    got = d_ids2[:int(d_ntok.item())].cpu().numpy().view(np.uint32)
    if (not np.array_equal(got, want[0]) or not np.array_equal(d_tok_off[:k + 1].cpu().numpy().view(np.uint64), want[1])
            or not np.array_equal(d_status2[:k].cpu().numpy(), want[2])):
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
    out = {"corpus": "S85k", "sentences": n_sent, "bytes": n_bytes, "vocabulary": len(vocab), "tokens_plain": n_plain, "tokens": tokens,
           "sentences_refused": refused, "checked_against_model": k, "rounds": args.rounds, "calls_per_window": reps, "legs": {}}
    for name, v in ms.items():
        med = statistics.median(v)
        out["legs"][name] = {"ms": [round(x, 4) for x in v], "median_ms": round(med, 4), "spread": round((max(v) - min(v)) / med, 4)}
    base = out["legs"]["plain"]["median_ms"]
    for name in [n for n in legs if n.startswith("dropout")]:
        out["legs"][name]["ratio_to_plain"] = round(out["legs"][name]["median_ms"] / base, 2)
    if "plain_parent" in legs:
        p = out["legs"]["plain_parent"]
        out["plain_against_parent"] = {"ratio": round(base / p["median_ms"], 4),
                                       "margin": round(max(p["spread"], out["legs"]["plain"]["spread"]), 4)}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a", encoding="utf-8") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
