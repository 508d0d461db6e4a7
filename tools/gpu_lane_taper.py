"""the tapering tiles of the FastBPE direct path (SWT_OPT_LANE_TAPER, csrc/swt_bpe_encode.hip: lane_map) against tiles of one size.

usage: python tools/gpu_lane_taper.py sweep [--passes P] [--settings 1,4,8,...] [--narrow V]
           bench.py's timed region of --workload bpe_encode (200 steps after 20, S85k resident in HBM, one perf_counter bracket
           round the steps) on S85k-open and S85k-lex for every setting in turn, P passes; beside it the lane kernel's own time
           from HIP events (swt_profile_read).  A setting is a value of SWT_OPT_LANE_TAPER: 1 = tiles of one size, v = 8 c, v + 256
           = 192 bytes as the smallest size.  --narrow V sets SWT_OPT_LANE_NARROW first (only where the library has the option):
           2 = the settings count from the narrow kernel's 512-byte tile, 1 = the wide kernel; setting 0 is the library's own choice.
       python tools/gpu_lane_taper.py midsize [--taper V] [--calls N] [--sizes KB,KB,...]
           one call at a time (launch, synchronize) on the first 64 KB, 256 KB, 1 MB and 2.5 MB of S85k-open, the median of N
           calls; without --taper the handle is left as the library made it, so the same file measures a parent's tree when it
           is run from there (cd parent && python <this file> midsize)."""
import argparse
import sys
import time

sys.path.insert(0, ".")
import numpy as np
import torch

from subword_tokenizers_amd import _native as N, synth, tokenizers

ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=["sweep", "midsize"])
ap.add_argument("--passes", type=int, default=2)
ap.add_argument("--settings", default="1,4,6,8,12,260,262,264,268")
ap.add_argument("--taper", type=int, default=None)
ap.add_argument("--narrow", type=int, default=None)
ap.add_argument("--sizes", default="64,256,1024,2560", help="midsize: the sizes in KB")
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--warmup", type=int, default=20)
args = ap.parse_args()

N.init(0)
bpe = tokenizers.FastBPE()
bpe.merges_list = list(synth.pretrained_merges()[:8000])
bpe._build_table()
h = bpe._table
if args.narrow is not None:
    h.set_option(7, args.narrow)  # SWT_OPT_LANE_NARROW
stream = torch.cuda.current_stream().cuda_stream


class Corpus:
    def __init__(self, sents):
        text, off = N.pack_utf8([s.lower() for s in sents])
        self.n_bytes, self.n_sent = int(text.size), len(sents)
        self.d_text = torch.from_numpy(text.copy()).cuda()
        self.d_off = torch.from_numpy(off.view(np.int64).copy()).cuda()
        self.d_out = torch.empty(self.n_bytes + 64, dtype=torch.int32, device="cuda")
        self.d_out_off = torch.empty(self.n_sent + 1, dtype=torch.int64, device="cuda")
        self.d_ntok = torch.zeros(1, dtype=torch.int64, device="cuda")

    def step(self):
        h.encode_dev(self.d_text.data_ptr(), self.n_bytes, self.d_off.data_ptr(), self.n_sent, self.d_out.data_ptr(),
                     self.d_out_off.data_ptr(), self.d_ntok.data_ptr(), 0, stream)

    def digest(self):
        n = int(self.d_ntok.item())
        return hash((self.d_out[:n].cpu().numpy().tobytes(), self.d_out_off.cpu().numpy().tobytes()))


def label(v):
    return "uniform" if v == 1 else "library" if v == 0 else "c=%.2f min %d" % ((v & ~256) / 8.0, 192 if v & 256 else 128)


if args.mode == "sweep":
    settings = [int(x) for x in args.settings.split(",")]
    for name, sents in (("S85k-open", synth.s85k_open()), ("S85k-lex", synth.s85k())):
        c = Corpus(sents)
        rows = {v: [] for v in settings}
        digests = set()
        for p in range(args.passes):
            for v in settings:
                h.set_option(N.OPT_LANE_TAPER, v)
                for _ in range(args.warmup):
                    c.step()
                torch.cuda.synchronize()
                N.profile_enable(True)
                N.profile_read()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    c.step()
                torch.cuda.synchronize()
                el = time.perf_counter() - t0
                ms, launches = N.profile_read()
                N.profile_enable(False)
                rows[v].append((el / args.steps * 1e3, ms / max(launches, 1) * 1e3))
                digests.add(c.digest())
        h.set_option(N.OPT_LANE_TAPER, 0)
        print("%s (%d bytes): ms per step | lane kernel us, %d passes; outputs identical: %s" % (name, c.n_bytes, args.passes, len(digests) == 1))
        for v in settings:
            print("  taper %3d  %-18s  %s  |  %s" % (v, label(v), "  ".join("%.4f" % a for a, _ in rows[v]), "  ".join("%.1f" % b for _, b in rows[v])))
else:
    sents = synth.s85k_open()
    if args.taper is not None:
        h.set_option(N.OPT_LANE_TAPER, args.taper)
    for size in [int(x) << 10 for x in args.sizes.split(",")]:
        take, total = [], 0
        for s in sents:
            take.append(s)
            total += len(s.encode("utf-8"))
            if total >= size:
                break
        c = Corpus(take)
        for _ in range(20):
            c.step()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.calls):
            t0 = time.perf_counter()
            c.step()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e6)
        ts = np.array(ts)
        print("midsize %8d bytes %6d sentences: median %.1f us  p10 %.1f  p90 %.1f  (taper %s)" % (c.n_bytes, c.n_sent, np.median(ts), np.percentile(ts, 10), np.percentile(ts, 90), args.taper))
