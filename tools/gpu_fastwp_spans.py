#!/usr/bin/env python3
"""What swt_wp_encode_spans_dev costs next to swt_wp_encode_dev (needs an MI355X; reads nothing but the package).

S85k-open resident in HBM, the pretrained WordPiece vocabulary.  Four calls alternate in one process, each timed with a pair of
HIP events around the one call; after --warmup rounds the figure of a call is the median of --repeats rounds:
  wp_encode_dev_nodedup      swt_wp_encode_dev with SWT_OPT_DEDUP = 1: the tiled path, which is the spans call's own (like for like)
  wp_encode_dev_shipped      swt_wp_encode_dev as shipped (the word-level dedup pipeline at this size)
  wp_encode_spans_dev_codepoints, wp_encode_spans_dev_bytes

Prints one JSON line: the medians with their spread ((max - min) / median), the output bytes (4 B per token for the id, 12 B on
top for the span and the word index), and the ratio of each spans leg to the two encode legs.  The ids of the spans call are
compared with the encode's.  With --out FILE the line is appended to FILE."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--sentences", type=int, default=85000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from subword_tokenizers_amd import _native as N
    from subword_tokenizers_amd import synth

    N.init(0)
    trie = N.WpTrie(sorted(set(synth.pretrained_vocab())))
    sents = synth.s85k_open(args.sentences)
    text, off = N.pack_utf8([s.lower() for s in sents])
    n_bytes, n_sent = int(text.size), len(sents)
    d_text = torch.from_numpy(np.concatenate([text, np.zeros(64, np.uint8)])).cuda()
    d_off = torch.from_numpy(off.view(np.int64)).cuda()
    d_ids = torch.empty(n_bytes + 64, dtype=torch.int32, device="cuda")
    d_ids2 = torch.empty(n_bytes + 64, dtype=torch.int32, device="cuda")
    d_tok_off = torch.empty(n_sent + 1, dtype=torch.int64, device="cuda")
    d_tok_off2 = torch.empty(n_sent + 1, dtype=torch.int64, device="cuda")
    d_status = torch.empty(n_sent, dtype=torch.uint8, device="cuda")
    d_ntok = torch.zeros(1, dtype=torch.int64, device="cuda")
    d_spans = torch.empty(2 * (n_bytes + 64), dtype=torch.int32, device="cuda")
    d_word = torch.empty(n_bytes + 64, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def encode(mode):
        trie.set_option(N.OPT_DEDUP, mode)
        trie.encode_dev(d_text.data_ptr(), n_bytes, d_off.data_ptr(), n_sent, d_ids.data_ptr(), d_tok_off.data_ptr(), d_status.data_ptr(),
                        d_ntok.data_ptr(), stream)

    def spans(codepoints):
        trie.encode_spans_dev(d_text.data_ptr(), n_bytes, d_off.data_ptr(), n_sent, d_ids2.data_ptr(), d_tok_off2.data_ptr(), d_status.data_ptr(),
                              d_ntok.data_ptr(), d_spans.data_ptr(), d_word.data_ptr(), codepoints=codepoints, stream=stream)

    legs = {"wp_encode_dev_nodedup": lambda: encode(N.DEDUP_NEVER), "wp_encode_dev_shipped": lambda: encode(N.DEDUP_AUTO),
            "wp_encode_spans_dev_codepoints": lambda: spans(True), "wp_encode_spans_dev_bytes": lambda: spans(False)}
    ms = {k: [] for k in legs}
    for r in range(args.warmup + args.repeats):
        for name, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r >= args.warmup:
                ms[name].append(e0.elapsed_time(e1))
    n_tok = int(d_ntok.item())
    assert torch.equal(d_ids[:n_tok], d_ids2[:n_tok]) and torch.equal(d_tok_off, d_tok_off2), "the spans call's ids differ from the encode's"
    # the spans of a sample against the strings (byte unit: the last leg)
    names = sorted(set(synth.pretrained_vocab()))
    sp = d_spans[:2 * 2000].cpu().numpy().reshape(-1, 2)
    ids = d_ids2[:2000].cpu().numpy().view(np.uint32)
    tok_off = d_tok_off2[:50].cpu().numpy()
    for s in range(40):
        low = sents[s].lower().encode("utf-8", "surrogatepass")
        for t in range(int(tok_off[s]), min(int(tok_off[s + 1]), 2000)):
            if int(ids[t]) < len(names):  # a vocabulary token: its span spells it, less the '##' of a later token of a segment
                body = names[int(ids[t])]
                got = low[sp[t, 0]:sp[t, 1]].decode("utf-8", "surrogatepass")
                assert got == body or (body.startswith("##") and got == body[2:]), (s, t, body, got)
    out = {"corpus": "S85k-open", "sentences": n_sent, "bytes": n_bytes, "tokens": n_tok, "vocab": len(names), "warmup": args.warmup,
           "repeats": args.repeats, "output_bytes": {"ids": 4 * n_tok, "spans_and_word": 12 * n_tok}, "legs": {}}
    for name, v in ms.items():
        med = statistics.median(v)
        out["legs"][name] = {"ms": [round(x, 4) for x in v], "median_ms": round(med, 4), "spread": round((max(v) - min(v)) / med, 4),
                             "text_gb_s": round(n_bytes / 1e6 / med, 1)}
    for name in ("wp_encode_spans_dev_codepoints", "wp_encode_spans_dev_bytes"):
        leg = out["legs"][name]
        leg["ratio_to_nodedup"] = round(leg["median_ms"] / out["legs"]["wp_encode_dev_nodedup"]["median_ms"], 3)
        leg["ratio_to_shipped"] = round(leg["median_ms"] / out["legs"]["wp_encode_dev_shipped"]["median_ms"], 3)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a", encoding="utf-8") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
