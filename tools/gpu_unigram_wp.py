#!/usr/bin/env python3
"""What the UnigramWP encode costs next to the plain NaiveWP encode, that the plain encode did not move, and what fit_scores takes
(needs an MI355X).

S85k, the pretrained 20,000-token vocabulary, scores from fit_scores(S85k, iterations=2), the lowercased text resident on the
device.  Legs that alternate round after round in one process, HIP events around enough back-to-back calls for 0.2 s each:
  plain          swt_wp_encode_naive_dev, this tree
  plain@X        the same call into another build of the library (--variant-lib X=PATH, repeatable)
  viterbi        swt_wp_encode_viterbi_dev
  dropout        swt_wp_encode_naive_dropout_dev at p = 0.1
  *_parent       the same three calls into the parent commit's library (--parent-lib, loaded beside this tree's), when one is given
Before the timing the Viterbi ids of the first --check sentences are compared with the model of tests/viterbi_cases.py.
Prints one JSON line; --out FILE appends it."""
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

NEEDED = ("swt_init", "swt_last_error", "swt_wp_trie_create", "swt_wp_trie_destroy", "swt_wp_encode_naive_dev")
DROPOUT = (round(0.1 * 2 ** 32), 0x5EED5EED5EED, 1)  # drop_below (p = 0.1), seed, epoch


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

    import subword_tokenizers_amd as S
    from subword_tokenizers_amd import _native as N
    from subword_tokenizers_amd import synth
    from tests import viterbi_cases as V

    N.init(0)
    sents = synth.s85k()[:args.sentences]
    tok = S.UnigramWP()
    tok.vocab = set(synth.pretrained_vocab())
    fit = {}
    for run in ("first", "second"):  # the first call builds the trie and loads the kernels
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        totals = tok.fit_scores(sents, iterations=2)
        e1.record(); e1.synchronize()
        fit[run] = {"wall_ms": round((time.perf_counter() - t0) * 1e3, 1), "between_events_ms": round(e0.elapsed_time(e1), 1), "tokens": totals}
    text, off = N.pack_and_lower(sents)
    n_bytes, n_sent = int(text.size), len(sents)
    stream = torch.cuda.current_stream().cuda_stream
    d_text = torch.from_numpy(np.concatenate([text, np.zeros(64, dtype=np.uint8)])).cuda()
    d_off = torch.from_numpy(off.view(np.int64)).cuda()
    d_ids = torch.zeros(n_bytes + 64, dtype=torch.int32, device="cuda")
    d_tok_off, d_ntok = torch.zeros(n_sent + 1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
    d_status = torch.zeros(n_sent + 8, dtype=torch.uint8, device="cuda")
    here, trie = N.lib(), tok._ensure_scored_trie()

    def call_of(lib, entry, h, draw=()):
        def call():
            if getattr(lib, entry)(h, d_text.data_ptr(), n_bytes, d_off.data_ptr(), n_sent, d_ids.data_ptr(), d_tok_off.data_ptr(),
                                   d_status.data_ptr(), d_ntok.data_ptr(), *draw, stream):
                raise RuntimeError("%s: %s" % (entry, lib.swt_last_error().decode()))
        return call

    legs = {"plain": call_of(here, "swt_wp_encode_naive_dev", trie._h), "viterbi": call_of(here, "swt_wp_encode_viterbi_dev", trie._h),
            "dropout": call_of(here, "swt_wp_encode_naive_dropout_dev", trie._h, DROPOUT)}
    blob, voff = N.pack_utf32(tok._naive_tokens)
    scores = np.array([tok.scores()[t] for t in tok._naive_tokens], dtype=np.float32)
    for leg, path in ([("plain_parent", args.parent_lib)] if args.parent_lib else []) + [("plain@" + v.partition("=")[0], v.partition("=")[2])
                                                                                         for v in args.variant_lib]:
        other = C.CDLL(os.path.abspath(path))
        for name in NEEDED:
            fn = getattr(other, name)
            fn.restype, fn.argtypes = N.SIGNATURES[name]
        if other.swt_init(0):
            raise RuntimeError("the library of %s does not initialise" % leg)
        h_other = C.c_void_p()
        if other.swt_wp_trie_create(N.ptr(blob, N.u32p), N.ptr(voff, N.u64p), len(tok._naive_tokens), C.byref(h_other)):
            raise RuntimeError("trie: %s" % other.swt_last_error().decode())
        legs[leg] = call_of(other, "swt_wp_encode_naive_dev", h_other)
        if leg == "plain_parent":
            for name in ("swt_wp_trie_set_scores", "swt_wp_encode_viterbi_dev", "swt_wp_encode_naive_dropout_dev"):
                fn = getattr(other, name)
                fn.restype, fn.argtypes = N.SIGNATURES[name]
            if other.swt_wp_trie_set_scores(h_other, N.ptr(scores, C.POINTER(C.c_float)), int(scores.size)):
                raise RuntimeError("scores: %s" % other.swt_last_error().decode())
            legs["viterbi_parent"] = call_of(other, "swt_wp_encode_viterbi_dev", h_other)
            legs["dropout_parent"] = call_of(other, "swt_wp_encode_naive_dropout_dev", h_other, DROPOUT)

    # ---- the check: the first k sentences as a call of their own against the model
    k = min(args.check, n_sent)
    d_off_k = d_off[:k + 1].clone()
    N.check(here.swt_wp_encode_viterbi_dev(trie._h, d_text.data_ptr(), int(off[k]), d_off_k.data_ptr(), k, d_ids.data_ptr(), d_tok_off.data_ptr(),
                                           d_status.data_ptr(), d_ntok.data_ptr(), stream))
    torch.cuda.synchronize()
    want = V.Model(tok.vocab, tok.scores()).batch(S.SubwordTokenizer._split, sents[:k])
    if (not np.array_equal(d_ids[:int(d_ntok.item())].cpu().numpy().view(np.uint32), want[0])
            or not np.array_equal(d_tok_off[:k + 1].cpu().numpy().view(np.uint64), want[1])):
        raise AssertionError("the Viterbi ids differ from the model on the first %d sentences" % k)
    tokens = {}
    for name in ("plain", "viterbi"):
        legs[name]()
        torch.cuda.synchronize()
        tokens[name] = int(d_ntok.item())

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
        for name, fn in legs.items():
            v = timed(fn, reps[name])
            if r >= args.warmup:
                ms[name].append(v)
    out = {"corpus": "S85k", "sentences": n_sent, "bytes": n_bytes, "vocabulary": len(tok.vocab), "tokens": tokens, "fit_scores": fit,
           "checked_against_model": k, "rounds": args.rounds, "calls_per_window": reps, "legs": {}}
    for name, v in ms.items():
        med = statistics.median(v)
        out["legs"][name] = {"ms": [round(x, 4) for x in v], "median_ms": round(med, 4), "spread": round((max(v) - min(v)) / med, 4)}
    base = out["legs"]["plain"]
    out["legs"]["viterbi"]["ratio_to_plain"] = round(out["legs"]["viterbi"]["median_ms"] / base["median_ms"], 2)
    for name in ("plain", "dropout", "viterbi"):
        if name + "_parent" in legs:
            p, mine = out["legs"][name + "_parent"], out["legs"][name]
            out[name + "_against_parent"] = {"ratio": round(mine["median_ms"] / p["median_ms"], 4), "margin": round(max(p["spread"], mine["spread"]), 4)}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a", encoding="utf-8") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
