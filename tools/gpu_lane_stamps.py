"""how the chip is filled over the life of bpe_lane_kernel's running-text form: the resident waves per CU against time, from the
begin / end stamps of every wave.  Needs a library built with SWT_EXTRA_FLAGS=-DSWT_STAMPS (csrc/swt_bpe_encode.hip: g_lane_stamp,
wall_clock64() at 100 MHz, two plain stores per wave).

usage: SWT_EXTRA_FLAGS=-DSWT_STAMPS python tools/gpu_lane_stamps.py [--lib PATH] [--taper V] [--slots N] [--span K] [open lex]
  --lib PATH   a stamps build elsewhere (a parent's, kept beside the tree's); default: build / load the tree's own
  --taper V    SWT_OPT_LANE_TAPER (only where the library has the option), --slots N SWT_OPT_LANE_SLOTS, --span K SWT_OPT_LANE_SPAN
One direct-path call per corpus (dedup off) after three warm calls.  Prints per corpus: the wave lives, the residency per CU in
2 us bins, the time of the last begin T_d, the last end, the steady-state residency before T_d, what the waves that end in the
last 30 us were given (tile index, life, span bytes, chunks), and whether begin times rise with blockIdx.x."""
import argparse
import ctypes
import os
import sys

sys.path.insert(0, ".")
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=None)
ap.add_argument("--taper", type=int, default=None)
ap.add_argument("--slots", type=int, default=None)
ap.add_argument("--span", type=int, default=None)
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
if not hasattr(L, "swt_debug_lane_stamps"):
    raise SystemExit("this library has no stamps: build it with SWT_EXTRA_FLAGS=-DSWT_STAMPS")
L.swt_debug_lane_stamps.argtypes = [ctypes.c_void_p]
has_map = hasattr(L, "swt_debug_bpe_tile_map")
if has_map:
    L.swt_debug_bpe_tile_map.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
n_stamps = L.swt_debug_lane_stamp_count() if hasattr(L, "swt_debug_lane_stamp_count") else 32768
CAP, TILE, CUS = 512, 384, torch.cuda.get_device_properties(0).multi_processor_count


def boundaries(handle, n_bytes):
    """first byte of every tile, and n_bytes behind them"""
    if has_map and args.span in (None, 0):
        m = np.zeros(13, dtype=np.uint64)
        assert L.swt_debug_bpe_tile_map(handle, n_bytes, m.ctypes.data) == 0
        n_tiles, segs = int(m[0]), m[1:].reshape(4, 3).astype(np.int64)
        print("  tile map: %d tiles; segments (first byte, first tile, tile bytes): %s" % (n_tiles, [tuple(s) for s in segs.tolist() if s[2]]))
        t = np.arange(n_tiles, dtype=np.int64)
        seg = np.zeros(n_tiles, dtype=np.int64)
        for k in range(1, 4):
            if segs[k][2]:
                seg[t >= segs[k][1]] = k
        b = segs[seg, 0] + (t - segs[seg, 1]) * segs[seg, 2]
    else:
        tile = TILE * (args.span or 1)
        b = np.arange(0, max(n_bytes, 1), tile, dtype=np.int64)
    return np.append(b, n_bytes)


def one(name):
    sents = synth.s85k() if name == "lex" else synth.s85k_open()
    bpe = tokenizers.FastBPE()
    bpe.merges_list = list(synth.pretrained_merges()[:8000])
    bpe._build_table()
    h = bpe._table
    h.set_option(N.OPT_DEDUP, N.DEDUP_NEVER)
    if args.span is not None:
        h.set_option(N.OPT_LANE_SPAN, args.span)
    if args.taper is not None:
        h.set_option(N.OPT_LANE_TAPER, args.taper)
    if args.slots is not None:
        h.set_option(N.OPT_LANE_SLOTS, args.slots)
    text, off = N.pack_utf8([s.lower() for s in sents])
    n_bytes, n_sent = int(text.size), len(sents)
    d_text = torch.from_numpy(text.copy()).cuda()
    d_off = torch.from_numpy(off.view(np.int64).copy()).cuda()
    d_out = torch.empty(n_bytes + 64, dtype=torch.int32, device="cuda")
    d_out_off = torch.empty(n_sent + 1, dtype=torch.int64, device="cuda")
    d_ntok = torch.zeros(1, dtype=torch.int64, device="cuda")
    stamps = np.zeros(2 * n_stamps, dtype=np.uint64)
    for i in range(4):
        if i == 3:
            assert L.swt_debug_lane_stamps(stamps.ctypes.data) == 0  # clears them
        h.encode_dev(d_text.data_ptr(), n_bytes, d_off.data_ptr(), n_sent, d_out.data_ptr(), d_out_off.data_ptr(), d_ntok.data_ptr(), 0, 0)
        torch.cuda.synchronize()
    assert L.swt_debug_lane_stamps(stamps.ctypes.data) == 0
    print("S85k-%s: %d bytes, %d sentences, %d tokens, %d CUs, taper %s slots %s span %s" % (name, n_bytes, n_sent, int(d_ntok.item()), CUS, args.taper, args.slots, args.span))
    bnd = boundaries(h._h, n_bytes)
    n_tiles = len(bnd) - 1
    assert n_tiles <= n_stamps, "more tiles than stamps: raise kLaneStamps"
    off = off.astype(np.int64)
    plan = np.searchsorted(off[:n_sent], bnd[:-1], side="left")
    plan = np.append(plan, n_sent)
    span = off[plan[1:]] - off[plan[:-1]]
    chunks = np.where(span > 0, 1 + (off[plan[1:]] - (off[plan[:-1]] & ~15) > CAP), 0)  # 1 or 2+ (a sentence longer than 2 chunks: "2")
    st = stamps.reshape(-1, 2)[:n_tiles].astype(np.float64) / 100.0  # us
    live = st[:, 1] > 0
    assert (live == (span > 0)).all(), "the stamps and the plan disagree on which tiles have work"
    t0 = st[live, 0].min()
    beg, end = st[:, 0] - t0, st[:, 1] - t0
    life = end - beg
    lv = life[live]
    t_d, t_e = beg[live].max(), end[live].max()
    print("  waves %d  sum of lives %.0f us  mean %.2f  p50 %.2f  p99 %.2f  max %.2f   first begin .. last end %.1f us   residency over the kernel %.1f per CU" % (
        live.sum(), lv.sum(), lv.mean(), np.median(lv), np.percentile(lv, 99), lv.max(), t_e, lv.sum() / t_e / CUS))
    print("  last begin T_d %.1f us   last end %.1f us   last end - T_d %.1f us" % (t_d, t_e, t_e - t_d))
    # residency: the mean number of resident waves per CU in each 2 us bin (the time a wave spends in the bin / 2 us / CUs)
    edges = np.arange(0.0, t_e + 2.0, 2.0)
    res = np.zeros(len(edges) - 1)
    for i in range(len(res)):
        res[i] = np.clip(np.minimum(end[live], edges[i + 1]) - np.maximum(beg[live], edges[i]), 0, None).sum() / 2.0 / CUS
    print("  resident waves per CU, 2 us bins from the first begin:")
    for i in range(0, len(res), 10):
        print("    %5.0f us  %s" % (edges[i], " ".join("%5.1f" % r for r in res[i:i + 10])))
    ramp = 10.0  # the first bins fill the chip
    sel = (edges[:-1] >= ramp) & (edges[1:] <= t_d)
    if sel.any():
        print("  steady state (%.0f us .. T_d): mean %.1f per CU, min %.1f, max %.1f" % (ramp, res[sel].mean(), res[sel].min(), res[sel].max()))
    sel = edges[:-1] >= t_d
    if sel.any():
        print("  drain (T_d .. last end): mean %.1f per CU;  empty slot-time against the steady state: drain %.0f, before T_d %.0f CU-slot-us" % (
            res[sel].mean(), ((res[(edges[:-1] >= ramp) & (edges[1:] <= t_d)].max() - res[sel]) * 2.0).clip(0).sum(),
            ((res[(edges[:-1] >= ramp) & (edges[1:] <= t_d)].max() - res[~sel]) * 2.0).clip(0).sum()))
    # the waves that end in the last 30 us
    tail = live & (end > t_e - 30.0)
    idx = np.nonzero(tail)[0]
    print("  waves that end in the last 30 us: %d (%d ran two chunks or more = %.1f %%; all waves: %.1f %%)" % (
        len(idx), (chunks[idx] > 1).sum(), 100.0 * (chunks[idx] > 1).mean(), 100.0 * (chunks[live] > 1).mean()))
    print("    tile index: min %d  p10 %d  p50 %d  p90 %d  max %d (of %d)" % (idx.min(), np.percentile(idx, 10), np.median(idx), np.percentile(idx, 90), idx.max(), n_tiles))
    print("    life: mean %.1f  p50 %.1f  p90 %.1f  max %.1f us    span bytes: mean %.0f  p90 %.0f  max %d" % (
        life[idx].mean(), np.median(life[idx]), np.percentile(life[idx], 90), life[idx].max(), span[idx].mean(), np.percentile(span[idx], 90), span[idx].max()))
    for lo in (10.0, 5.0, 2.0):
        j = np.nonzero(live & (end > t_e - lo))[0]
        print("    ending in the last %4.1f us: %5d waves, life mean %.1f us, begin mean %.1f us, two chunks %.0f %%" % (lo, len(j), life[j].mean(), beg[j].mean(), 100.0 * (chunks[j] > 1).mean()))
    print("  life by chunks: one %.1f us (%d waves), two or more %.1f us (%d waves)" % (
        life[live & (chunks == 1)].mean(), (live & (chunks == 1)).sum(), life[chunks > 1].mean() if (chunks > 1).any() else 0.0, (chunks > 1).sum()))
    # do begin times rise with blockIdx.x?
    li = np.nonzero(live)[0]
    r = np.corrcoef(li, beg[li])[0, 1]
    order = np.argsort(beg[li], kind="stable")
    disp = np.abs(np.argsort(order) - np.arange(len(li)))  # how far a wave's rank by begin time is from its rank by index
    print("  begin against blockIdx.x: correlation %.4f; rank displacement mean %.0f, p99 %.0f, max %d waves (slots: about %d)" % (
        r, disp.mean(), np.percentile(disp, 99), disp.max(), int(res.max() * CUS)))
    for q in range(8):
        a, b = q * len(li) // 8, (q + 1) * len(li) // 8
        print("    tiles %6d..%6d: begin mean %6.1f  min %6.1f  max %6.1f   life mean %.1f" % (li[a], li[b - 1], beg[li[a:b]].mean(), beg[li[a:b]].min(), beg[li[a:b]].max(), life[li[a:b]].mean()))
    h.set_option(N.OPT_DEDUP, N.DEDUP_AUTO)


for c in args.corpora:
    one(c)
