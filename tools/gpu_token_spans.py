#!/usr/bin/env python3
"""What swt_token_spans_dev costs next to the encode that made its ids (needs an MI355X; reads nothing but the package).

S85k-open resident in HBM, FastBPE ids of the 8,000-merge table of bench.py's encode config.  Three calls alternate in one
process -- swt_bpe_encode_dev, swt_token_spans_dev in code points, swt_token_spans_dev in bytes -- each timed with a pair of HIP
events around the one call; after --warmup rounds the figure of a call is the median of --repeats rounds.

Prints one JSON line: the three medians with their spread ((max - min) / median), the algorithmic bytes of the span pass (text +
4 B per id in, 8 B span + 4 B word index per token out: 8 to 12 B), what that is per second, and the ratio to the encode.
With --out FILE the line is appended to FILE."""
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
    from subword_tokenizers_amd import synth, tokenizers

    N.init(0)
    tok = tokenizers.FastBPE()
    tok.merges_list = list(synth.pretrained_merges()[:8000])
    tok._build_table()
    table = tok._ensure_table()
    sents = synth.s85k_open(args.sentences)
    text, off = N.pack_utf8([s.lower() for s in sents])
    n_bytes, n_sent = int(text.size), len(sents)
    lengths = tok._span_lengths(tok._syms)
    d_text = torch.from_numpy(np.concatenate([text, np.zeros(64, np.uint8)])).cuda()
    d_off = torch.from_numpy(off.view(np.int64)).cuda()
    d_ids = torch.empty(n_bytes + 64, dtype=torch.int32, device="cuda")
    d_tok_off = torch.empty(n_sent + 1, dtype=torch.int64, device="cuda")
    d_ntok = torch.zeros(1, dtype=torch.int64, device="cuda")
    d_len = torch.from_numpy(np.concatenate([lengths, np.zeros(4, np.uint32)]).view(np.int32)).cuda()
    stream = torch.cuda.current_stream().cuda_stream

    def encode():
        table.encode_dev(d_text.data_ptr(), n_bytes, d_off.data_ptr(), n_sent, d_ids.data_ptr(), d_tok_off.data_ptr(), d_ntok.data_ptr(), 0, stream)

    encode()
    torch.cuda.synchronize()
    n_tok = int(d_ntok.item())
    d_spans = torch.empty(2 * n_tok, dtype=torch.int32, device="cuda")
    d_word = torch.empty(n_tok, dtype=torch.int32, device="cuda")
    d_status = torch.empty(n_sent, dtype=torch.uint8, device="cuda")

    def spans(flags):
        N.check(N.lib().swt_token_spans_dev(d_text.data_ptr(), n_bytes, d_off.data_ptr(), n_sent, d_ids.data_ptr(), d_tok_off.data_ptr(),
                                            d_len.data_ptr(), N.SYM_BASE, int(lengths.size), 1, flags, d_spans.data_ptr(), d_word.data_ptr(),
                                            d_status.data_ptr(), stream))

    legs = {"bpe_encode_dev": encode, "token_spans_dev_codepoints": lambda: spans(N.SPAN_CODEPOINTS), "token_spans_dev_bytes": lambda: spans(0)}
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
    assert not bool(d_status.any().item()), "a sentence's ids do not tile its text"
    # the spans of a sample against the strings
    sp = d_spans[:2 * 2000].cpu().numpy().reshape(-1, 2)
    ids = d_ids[:2000].cpu().numpy().view(np.uint32)
    tok_off = d_tok_off[:50].cpu().numpy()
    for s in range(40):
        low = sents[s].lower().encode("utf-8", "surrogatepass")
        for t in range(int(tok_off[s]), min(int(tok_off[s + 1]), 2000)):
            body = tok._syms.string(int(ids[t]))
            assert low[sp[t, 0]:sp[t, 1]].decode("utf-8", "surrogatepass") == body, (s, t)
    algo = {"in": n_bytes + 4 * n_tok, "out_min": 8 * n_tok, "out_max": 12 * n_tok}
    out = {"corpus": "S85k-open", "sentences": n_sent, "bytes": n_bytes, "tokens": n_tok, "merges": len(tok.merges_list),
           "warmup": args.warmup, "repeats": args.repeats, "algorithmic_bytes": algo, "legs": {}}
    for name, v in ms.items():
        med = statistics.median(v)
        out["legs"][name] = {"ms": [round(x, 4) for x in v], "median_ms": round(med, 4), "spread": round((max(v) - min(v)) / med, 4),
                             "text_gb_s": round(n_bytes / 1e6 / med, 1)}
    enc = out["legs"]["bpe_encode_dev"]["median_ms"]
    for name in ("token_spans_dev_codepoints", "token_spans_dev_bytes"):
        leg = out["legs"][name]
        leg["ratio_to_encode"] = round(leg["median_ms"] / enc, 3)
        leg["algorithmic_gb_s"] = round((algo["in"] + algo["out_max"]) / 1e6 / leg["median_ms"], 1)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a", encoding="utf-8") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
