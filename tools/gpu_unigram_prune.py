#!/usr/bin/env python3
"""What the removal losses (swt_wp_removal_losses_dev) cost next to the Viterbi encode, whose forward pass they repeat per word; that
the Viterbi encode did not move; and what train_unigram does with them (needs an MI355X).

S85k, the pretrained 20,000-token vocabulary, scores from fit_scores(S85k, iterations=2), the lowercased text resident on the
device.  Legs that alternate round after round in one process, HIP events around enough back-to-back calls for 0.2 s each:
  prune            swt_wp_removal_losses_dev
  viterbi          swt_wp_encode_viterbi_dev
  *_parent         both calls into the parent commit's library (--parent-lib, loaded beside this tree's)
Before the timing the table and stats of the first --check sentences are compared with the model of tests/prune_cases.py.  Then
train_unigram from the pretrained vocabulary as the seed down to --target on the first --train sentences, wall clock.  Prints one
JSON line; --out FILE appends it."""
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
    ap.add_argument("--sentences", type=int, default=85000)
    ap.add_argument("--check", type=int, default=300)
    ap.add_argument("--train", type=int, default=20000)
    ap.add_argument("--target", type=int, default=8000)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import subword_tokenizers_amd as S
    from subword_tokenizers_amd import _native as N
    from subword_tokenizers_amd import synth
    from tests import prune_cases as P

    N.init(0)
    sents = synth.s85k()[:args.sentences]
    tok = S.UnigramWP()
    tok.vocab = set(synth.pretrained_vocab())
    tok.fit_scores(sents, iterations=2)
    text, off = N.pack_and_lower(sents)
    n_bytes, n_sent, size = int(text.size), len(sents), len(tok.vocab)
    stream = torch.cuda.current_stream().cuda_stream
    d_text = torch.from_numpy(np.concatenate([text, np.zeros(64, dtype=np.uint8)])).cuda()
    d_off = torch.from_numpy(off.view(np.int64)).cuda()
    d_ids = torch.zeros(n_bytes + 64, dtype=torch.int32, device="cuda")
    d_tok_off, d_ntok = torch.zeros(n_sent + 1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
    d_status = torch.zeros(n_sent + 8, dtype=torch.uint8, device="cuda")
    d_table = torch.zeros(3 * size + 3, dtype=torch.int64, device="cuda")
    here, trie = N.lib(), tok._ensure_scored_trie()
    scores = np.array([tok.scores()[t] for t in tok._naive_tokens], dtype=np.float32)

    def viterbi_of(lib, h):
        def call():
            if lib.swt_wp_encode_viterbi_dev(h, d_text.data_ptr(), n_bytes, d_off.data_ptr(), n_sent, d_ids.data_ptr(), d_tok_off.data_ptr(),
                                             d_status.data_ptr(), d_ntok.data_ptr(), stream):
                raise RuntimeError("swt_wp_encode_viterbi_dev: %s" % lib.swt_last_error().decode())
        return call

    def prune(k=n_sent, d_off_k=d_off):
        trie.removal_losses_dev(d_text.data_ptr(), int(off[k]), d_off_k.data_ptr(), k, d_table[3:].data_ptr(), d_table.data_ptr(), stream)

    legs = {"prune": prune, "viterbi": viterbi_of(here, trie._h)}
    if args.parent_lib:
        other = C.CDLL(os.path.abspath(args.parent_lib))
        for name in ("swt_init", "swt_last_error", "swt_wp_trie_create", "swt_wp_trie_set_scores", "swt_wp_encode_viterbi_dev",
                     "swt_wp_removal_losses_dev"):
            fn = getattr(other, name)
            fn.restype, fn.argtypes = N.SIGNATURES[name]
        blob, voff = N.pack_utf32(tok._naive_tokens)
        h = C.c_void_p()
        if (other.swt_init(0) or other.swt_wp_trie_create(N.ptr(blob, N.u32p), N.ptr(voff, N.u64p), size, C.byref(h))
                or other.swt_wp_trie_set_scores(h, N.ptr(scores, C.POINTER(C.c_float)), size)):
            raise RuntimeError("the parent's library: %s" % other.swt_last_error().decode())
        legs["viterbi_parent"] = viterbi_of(other, h)

        def prune_parent():
            if other.swt_wp_removal_losses_dev(h, d_text.data_ptr(), n_bytes, d_off.data_ptr(), n_sent, d_table[3:].data_ptr(),
                                               d_table.data_ptr(), stream):
                raise RuntimeError("swt_wp_removal_losses_dev: %s" % other.swt_last_error().decode())
        legs["prune_parent"] = prune_parent

    # ---- the check: the first k sentences as a call of their own against the model
    k = min(args.check, n_sent)
    prune(k, d_off[:k + 1].clone())
    got = d_table.cpu().numpy()
    want = P.Prune(tok.vocab, tok.scores()).batch(S.SubwordTokenizer._split, sents[:k])
    if not np.array_equal(got[3:].view(np.uint64).reshape(3, size), want[0]) or not np.array_equal(got[:3], want[1]):
        raise AssertionError("the table or the stats differ from the model on the first %d sentences" % k)
    prune()
    legs["viterbi"]()
    torch.cuda.synchronize()
    table, stats = d_table[3:].cpu().numpy().reshape(3, size), d_table[:3].tolist()

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
    out = {"corpus": "S85k", "sentences": n_sent, "bytes": n_bytes, "vocabulary": size, "viterbi_tokens": int(d_ntok.item()), "words": stats[0],
           "unk_words": stats[1], "viterbi_total_nats": stats[2] * 2.0 ** -20, "pieces_in_use": int(np.count_nonzero(table[0])),
           "pieces_with_a_loss": int(np.count_nonzero(table[1])), "pieces_that_orphan": int(np.count_nonzero(table[2])),
           "checked_against_model": k, "rounds": args.rounds, "calls_per_window": reps, "legs": {}}
    for name, v in ms.items():
        med = statistics.median(v)
        out["legs"][name] = {"ms": [round(x, 4) for x in v], "median_ms": round(med, 4), "spread": round((max(v) - min(v)) / med, 4)}
    leg = out["legs"]
    leg["prune"]["ratio_to_viterbi"] = round(leg["prune"]["median_ms"] / leg["viterbi"]["median_ms"], 3)
    for name in ("prune", "viterbi"):
        if name + "_parent" in leg:
            p = leg[name + "_parent"]
            out[name + "_against_parent"] = {"ratio": round(leg[name]["median_ms"] / p["median_ms"], 4), "margin": round(max(p["spread"], leg[name]["spread"]), 4)}

    # ---- the trainer, the pretrained vocabulary as its seed, on a tokenizer of its own
    fresh = S.UnigramWP()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rounds = fresh.train_unigram(sents[:args.train], args.target, seed_vocab=tok.vocab)
    out["train_unigram"] = {"sentences": min(args.train, n_sent), "target": args.target, "wall_s": round(time.perf_counter() - t0, 3),
                            "rounds": rounds, "final_vocabulary": len(fresh.vocab)}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a", encoding="utf-8") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
