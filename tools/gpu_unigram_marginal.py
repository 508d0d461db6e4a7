#!/usr/bin/env python3
"""What the E-step of soft EM (swt_wp_expected_counts_dev) costs next to the sampled encode, which makes the same two lattice walks,
and next to one hard iteration; that the Viterbi and the sampled encode did not move; and what four soft iterations give (needs an
MI355X).

S85k, the pretrained 20,000-token vocabulary, scores from fit_scores(S85k, iterations=2), weights at alpha 1, the lowercased text
resident on the device.  Legs that alternate round after round in one process, HIP events around enough back-to-back calls for
0.2 s each:
  marginal         swt_wp_expected_counts_dev
  sample           swt_wp_encode_sample_dev
  hard             swt_wp_encode_viterbi_dev and swt_token_histogram_dev over its ids: the E-step of one hard iteration
  viterbi          swt_wp_encode_viterbi_dev
  *_parent         the marginal, the sampled and the Viterbi call into the parent commit's library (--parent-lib, loaded beside
                   this tree's)
Before the timing the counts and stats of the first --check sentences are compared with the model of tests/marginal_cases.py.
Then fit_scores(method="soft", iterations=--soft) on a fresh tokenizer, wall clock.  Prints one JSON line; --out FILE appends it."""
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

SEED, EPOCH = 0x5EED5EED5EED, 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sentences", type=int, default=85000)
    ap.add_argument("--check", type=int, default=300)
    ap.add_argument("--soft", type=int, default=4)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import subword_tokenizers_amd as S
    from subword_tokenizers_amd import _native as N
    from subword_tokenizers_amd import synth
    from tests import marginal_cases as M

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
    d_counts, d_hist = torch.zeros(size + 3, dtype=torch.int64, device="cuda"), torch.zeros(2 * (size + 2) + 1, dtype=torch.int64, device="cuda")
    here, trie = N.lib(), tok._ensure_scored_trie()
    scores = np.array([tok.scores()[t] for t in tok._naive_tokens], dtype=np.float32)
    weights = N.sample_weights(scores, 1.0)
    trie.set_weights(weights)

    def encode_of(lib, entry, h, draw=()):
        def call():
            if getattr(lib, entry)(h, d_text.data_ptr(), n_bytes, d_off.data_ptr(), n_sent, d_ids.data_ptr(), d_tok_off.data_ptr(),
                                   d_status.data_ptr(), d_ntok.data_ptr(), *draw, stream):
                raise RuntimeError("%s: %s" % (entry, lib.swt_last_error().decode()))
        return call

    def marginal(k=n_sent, d_off_k=d_off, lib=here, h=trie._h):
        if lib.swt_wp_expected_counts_dev(h, d_text.data_ptr(), int(off[k]), d_off_k.data_ptr(), k, d_counts[3:].data_ptr(),
                                          d_counts.data_ptr(), stream):
            raise RuntimeError("swt_wp_expected_counts_dev: %s" % lib.swt_last_error().decode())

    viterbi = encode_of(here, "swt_wp_encode_viterbi_dev", trie._h)
    viterbi()
    torch.cuda.synchronize()
    n_tok = int(d_ntok.item())

    def hard():
        viterbi()
        N.check(here.swt_token_histogram_dev(d_ids.data_ptr(), n_tok, size + 2, d_hist[1:].data_ptr(), d_hist.data_ptr(), stream))

    legs = {"marginal": marginal, "sample": encode_of(here, "swt_wp_encode_sample_dev", trie._h, (SEED, EPOCH)), "hard": hard, "viterbi": viterbi}
    if args.parent_lib:
        other = C.CDLL(os.path.abspath(args.parent_lib))
        for name in ("swt_init", "swt_last_error", "swt_wp_trie_create", "swt_wp_trie_set_scores", "swt_wp_trie_set_weights",
                     "swt_wp_encode_viterbi_dev", "swt_wp_encode_sample_dev", "swt_wp_expected_counts_dev"):
            fn = getattr(other, name)
            fn.restype, fn.argtypes = N.SIGNATURES[name]
        blob, voff = N.pack_utf32(tok._naive_tokens)
        h = C.c_void_p()
        if (other.swt_init(0) or other.swt_wp_trie_create(N.ptr(blob, N.u32p), N.ptr(voff, N.u64p), size, C.byref(h))
                or other.swt_wp_trie_set_scores(h, N.ptr(scores, C.POINTER(C.c_float)), size)
                or other.swt_wp_trie_set_weights(h, N.ptr(weights, C.POINTER(C.c_float)), size)):
            raise RuntimeError("the parent's library: %s" % other.swt_last_error().decode())
        legs["sample_parent"] = encode_of(other, "swt_wp_encode_sample_dev", h, (SEED, EPOCH))
        legs["viterbi_parent"] = encode_of(other, "swt_wp_encode_viterbi_dev", h)
        legs["marginal_parent"] = lambda: marginal(lib=other, h=h)

    # ---- the check: the first k sentences as a call of their own against the model
    k = min(args.check, n_sent)
    marginal(k, d_off[:k + 1].clone())
    got = d_counts.cpu().numpy()
    want = M.Marginal(tok.vocab, dict(zip(tok._naive_tokens, weights))).batch(S.SubwordTokenizer._split, sents[:k])
    if not np.array_equal(got[3:].view(np.uint64), want[0]) or not np.array_equal(got[:3], want[1]):
        raise AssertionError("the counts or the stats differ from the model on the first %d sentences" % k)
    marginal()
    stats = d_counts[:3].tolist()

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
    out = {"corpus": "S85k", "sentences": n_sent, "bytes": n_bytes, "vocabulary": size, "viterbi_tokens": n_tok, "words": stats[0],
           "unk_words": stats[1], "log2_likelihood": stats[2] * 2.0 ** -24, "checked_against_model": k, "rounds": args.rounds,
           "calls_per_window": reps, "legs": {}}
    for name, v in ms.items():
        med = statistics.median(v)
        out["legs"][name] = {"ms": [round(x, 4) for x in v], "median_ms": round(med, 4), "spread": round((max(v) - min(v)) / med, 4)}
    leg = out["legs"]
    for base in ("sample", "hard"):
        leg["marginal"]["ratio_to_" + base] = round(leg["marginal"]["median_ms"] / leg[base]["median_ms"], 3)
    for name in ("marginal", "sample", "viterbi"):
        if name + "_parent" in leg:
            p = leg[name + "_parent"]
            out[name + "_against_parent"] = {"ratio": round(leg[name]["median_ms"] / p["median_ms"], 4), "margin": round(max(p["spread"], leg[name]["spread"]), 4)}

    # ---- soft EM from the same hard start, on a tokenizer of its own
    soft = S.UnigramWP()
    soft.vocab = set(tok.vocab)
    soft.set_scores(tok.scores())
    soft.fit_scores(sents[:1000], iterations=1, method="soft")  # (warm-up; the scores are put back)
    soft.set_scores(tok.scores())
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    likes = soft.fit_scores(sents, iterations=args.soft, method="soft")
    out["soft_fit"] = {"iterations": args.soft, "wall_s": round(time.perf_counter() - t0, 3), "log2_likelihood": likes,
                       "rises": all(b > a for a, b in zip(likes, likes[1:]))}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a", encoding="utf-8") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
