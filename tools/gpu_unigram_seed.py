#!/usr/bin/env python3
"""What the substring census (swt_substring_counts_text_dev) costs, what UnigramWP.seed_substrings costs next to today's seed
(NaiveWP.train), what train_unigram makes of each seed, and that the Viterbi encode did not move (needs an MI355X).

The first --sentences sentences of S85k.  The counts of the first --check sentences are compared with the model of
tests/seed_cases.py first.  Then, in one process:
  kernels   HIP events (swt_profile_enable) around the insert kernel (1) and around all kernels of the census (2: the sizing pass,
            the fill, the inserts, select, scan and emit; not the word census in front of them), min_count = 1 so that every distinct
            key comes back, --rounds calls each after --warmup
  seeds     wall clock of seed_substrings(sents, --seed-size) and of NaiveWP.train(sents, --seed-size), each ending in a synchronise
  trainers  train_unigram(sents, --target) with each seed: wall clock, the last round's viterbi_total and unk_words, and the
            log2-likelihood of expected_counts at the end
  viterbi   swt_wp_encode_viterbi_dev under the substring trainer's vocabulary, this tree's library and the parent commit's
            (--parent-lib, loaded beside it) alternating round after round, enough back-to-back calls for 0.2 s each
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sentences", type=int, default=20000)
    ap.add_argument("--check", type=int, default=300)
    ap.add_argument("--seed-size", type=int, default=32000)
    ap.add_argument("--target", type=int, default=8000)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import subword_tokenizers_amd as S
    from subword_tokenizers_amd import _native as N
    from subword_tokenizers_amd import synth
    from tests import seed_cases as M

    N.init(0)
    sents = synth.s85k()[:args.sentences]
    tok = S.UnigramWP()

    # ---- the check: the first k sentences against the model
    k = min(args.check, len(sents))
    words = [(w, 1) for s in tok.preprocessing([t.lower() for t in sents[:k]]) for w, _ in s]
    want = {M.token(key): v for key, v in M.census(words, 16, 2, tok.max_word_chars).items()}
    if tok.seed_substrings(sents[:k], 10 ** 9, return_counts=True)[1] != want:
        raise AssertionError("the counts differ from the model on the first %d sentences" % k)

    # ---- the kernels
    d_text, n_bytes, d_off, dev, stream = tok._resident(sents)
    syms, woff, freq = N.BpeTrainer.from_text(*N.pack_and_lower(sents)).export()
    wlen = np.diff(woff.astype(np.int64))
    wlen = wlen[wlen <= tok.max_word_chars]
    insertions = int(sum((np.minimum(16, wlen - i) - 1).clip(0).sum() for i in range(int(wlen.max(initial=0)))))  # per start i: lengths 2..
    cap = 2 * insertions + 16
    outs = [torch.empty(cap + 1, dtype=torch.int64, device=dev), torch.empty(16 * cap, dtype=torch.int32, device=dev),
            torch.empty(cap, dtype=torch.uint8, device=dev), torch.empty(cap, dtype=torch.int64, device=dev)]

    def census():
        rc, n, m, _ = N.substring_counts_text_dev(d_text.data_ptr(), n_bytes, d_off.data_ptr(), len(sents), 16, 1, tok.max_word_chars,
                                                  [t.data_ptr() for t in outs], cap, 16 * cap, 0, stream)
        N.check(rc)
        return n

    kernels = {}
    for level, name in ((1, "insert_kernel_ms"), (2, "all_kernels_ms")):
        got = []
        for r in range(args.warmup + args.rounds):
            N.profile_enable(level)
            distinct = census()
            ms, brackets = N.profile_read()
            N.profile_enable(False)
            if r >= args.warmup:
                got.append(ms)
        kernels[name] = {"ms": [round(x, 4) for x in got], "median_ms": round(statistics.median(got), 4), "brackets_per_call": brackets}
    kernels.update(unique_words=int(freq.size), insertions=insertions, distinct_keys=distinct,
                   insertions_per_s=round(insertions / (kernels["insert_kernel_ms"]["median_ms"] * 1e-3)))
    del outs

    # ---- the two seeds, then the trainer on each
    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = fn()
        torch.cuda.synchronize()
        return got, round(time.perf_counter() - t0, 3)

    tok.seed_substrings(sents[:k], 100)  # (warm: code objects, torch's allocator)
    seed, seed_s = wall(lambda: tok.seed_substrings(sents, args.seed_size))
    merges = S.NaiveWP()
    _, merges_s = wall(lambda: merges.train(sents, args.seed_size))
    out = {"corpus": "S85k", "sentences": len(sents), "bytes": n_bytes, "checked_against_model": k, "kernels": kernels,
           "seed": {"size": args.seed_size, "substrings_wall_s": seed_s, "substrings_tokens": len(seed), "merges_wall_s": merges_s,
                    "merges_tokens": len(merges.vocab), "common_tokens": len(set(seed) & merges.vocab)}, "train_unigram": {}}
    trained = {}
    for name in ("merges", "substrings"):
        trained[name] = S.UnigramWP()
        rounds, secs = wall(lambda: trained[name].train_unigram(sents, args.target, seed=name))
        end, like = trained[name].removal_losses(sents), trained[name].expected_counts(sents)
        out["train_unigram"][name] = {"wall_s": secs, "rounds": len(rounds), "seed_vocabulary": rounds[0][0] if rounds else None,
                                      "final_vocabulary": len(trained[name].vocab), "viterbi_total_nats": end["viterbi_total"],
                                      "unk_words": end["unk_words"], "log2_likelihood": like["log2_likelihood"]}

    # ---- the Viterbi encode, which this change does not touch, against the parent's library
    if args.parent_lib:
        t = trained["substrings"]
        trie, size, n_sent = t._ensure_scored_trie(), len(t.vocab), len(sents)
        scores = np.array([t.scores()[x] for x in t._naive_tokens], dtype=np.float32)
        d_ids = torch.zeros(n_bytes + 64, dtype=torch.int32, device=dev)
        d_tok_off, d_ntok = torch.zeros(n_sent + 1, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
        d_status = torch.zeros(n_sent + 8, dtype=torch.uint8, device=dev)
        other = C.CDLL(os.path.abspath(args.parent_lib))
        for fn_name in ("swt_init", "swt_last_error", "swt_wp_trie_create", "swt_wp_trie_set_scores", "swt_wp_encode_viterbi_dev"):
            fn = getattr(other, fn_name)
            fn.restype, fn.argtypes = N.SIGNATURES[fn_name]
        blob, voff = N.pack_utf32(t._naive_tokens)
        h = C.c_void_p()
        if (other.swt_init(0) or other.swt_wp_trie_create(N.ptr(blob, N.u32p), N.ptr(voff, N.u64p), size, C.byref(h))
                or other.swt_wp_trie_set_scores(h, N.ptr(scores, C.POINTER(C.c_float)), size)):
            raise RuntimeError("the parent's library: %s" % other.swt_last_error().decode())

        def viterbi_of(lib, handle):
            def call():
                if lib.swt_wp_encode_viterbi_dev(handle, d_text.data_ptr(), n_bytes, d_off.data_ptr(), n_sent, d_ids.data_ptr(),
                                                 d_tok_off.data_ptr(), d_status.data_ptr(), d_ntok.data_ptr(), stream):
                    raise RuntimeError("swt_wp_encode_viterbi_dev: %s" % lib.swt_last_error().decode())
            return call

        def timed(fn, reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record(); e1.synchronize()
            return e0.elapsed_time(e1) / reps

        legs = {"viterbi": viterbi_of(N.lib(), trie._h), "viterbi_parent": viterbi_of(other, h)}
        reps = {name: max(1, int(np.ceil(200.0 / max(timed(fn, 10), 1e-3)))) for name, fn in legs.items()}
        ms = {name: [] for name in legs}
        for r in range(args.warmup + args.rounds):
            for name, fn in legs.items():
                v = timed(fn, reps[name])
                if r >= args.warmup:
                    ms[name].append(v)
        leg = {name: {"ms": [round(x, 4) for x in v], "median_ms": round(statistics.median(v), 4),
                      "spread": round((max(v) - min(v)) / statistics.median(v), 4)} for name, v in ms.items()}
        out["viterbi_against_parent"] = dict(leg, ratio=round(leg["viterbi"]["median_ms"] / leg["viterbi_parent"]["median_ms"], 4),
                                             margin=round(max(x["spread"] for x in leg.values()), 4))
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a", encoding="utf-8") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
