"""how many trips the scan loops of the narrow bpe_lane_kernel make as the WAVE executes them (a trip costs the wave the same
whether one lane takes part or sixty): when a lane takes a word, after a round, and in the tail of the rounds.  Needs a library
built with SWT_EXTRA_FLAGS=-DSWT_SCAN_TRIPS (csrc/swt_bpe_encode.hip: g_scan_trips, one atomic add per trip by its first active
lane -- the counts are exact, the kernel's time under this build means nothing).

usage: SWT_EXTRA_FLAGS=-DSWT_SCAN_TRIPS python tools/gpu_lane_keys.py [--lib PATH] [--valu N] [open lex]
  --lib PATH   a counting build elsewhere; default: build / load the tree's own
  --valu N     vector instructions per trip of the build that is being judged (the static count from its .s), for the share
One direct-path call per corpus (dedup off) after two warm calls.  Prints per corpus the three counts per launch and per input byte."""
import argparse
import ctypes
import os
import sys

sys.path.insert(0, ".")
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=None)
ap.add_argument("--valu", type=float, default=None)
ap.add_argument("corpora", nargs="*", default=["open", "lex"])
args = ap.parse_args()

import torch
from subword_tokenizers_amd import _build as B, _native as N, synth, tokenizers

if args.lib:
    B.LIB_PATH = os.path.abspath(args.lib)  # before the first N.lib()
else:
    B.build()

N.init(0)
L = ctypes.CDLL(B.LIB_PATH)
if not hasattr(L, "swt_debug_scan_trips"):
    raise SystemExit("this library does not count: build it with SWT_EXTRA_FLAGS=-DSWT_SCAN_TRIPS")
L.swt_debug_scan_trips.argtypes = [ctypes.c_void_p]
L.swt_debug_bpe_table_info.restype, L.swt_debug_bpe_table_info.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]

for name in args.corpora:
    sents = synth.s85k() if name == "lex" else synth.s85k_open()
    bpe = tokenizers.FastBPE()
    bpe.merges_list = list(synth.pretrained_merges()[:8000])
    bpe._build_table()
    h = bpe._table
    h.set_option(N.OPT_DEDUP, N.DEDUP_NEVER)
    text, off = N.pack_utf8([s.lower() for s in sents])
    n_bytes, n_sent = int(text.size), len(sents)
    d_text = torch.from_numpy(text.copy()).cuda()
    d_off = torch.from_numpy(off.view(np.int64).copy()).cuda()
    d_out = torch.empty(n_bytes + 64, dtype=torch.int32, device="cuda")
    d_out_off = torch.empty(n_sent + 1, dtype=torch.int64, device="cuda")
    d_ntok = torch.zeros(1, dtype=torch.int64, device="cuda")
    trips = np.zeros(3, dtype=np.uint64)
    for i in range(3):
        if i == 2:
            assert L.swt_debug_scan_trips(trips.ctypes.data) == 0  # clears them
        h.encode_dev(d_text.data_ptr(), n_bytes, d_off.data_ptr(), n_sent, d_out.data_ptr(), d_out_off.data_ptr(), d_ntok.data_ptr(), 0, 0)
        torch.cuda.synchronize()
    assert L.swt_debug_scan_trips(trips.ctypes.data) == 0
    assert L.swt_debug_bpe_table_info(h._h, 11) == 1, "the call did not take the narrow kernel"
    take, rnd, tail = (int(x) for x in trips)
    total = take + rnd + tail
    print("S85k-%s: %d bytes, %d tokens; scan trips per launch: take %d  after a round %d  tail %d  (a tail trip is one group of four slots)  total %d = %.4f per byte"
          % (name, n_bytes, int(d_ntok.item()), take, rnd, tail, total, total / n_bytes))
    if args.valu:
        print("  at %.1f vector instructions a trip: %.0f vector instructions = %.3f per byte" % (args.valu, total * args.valu, total * args.valu / n_bytes))
