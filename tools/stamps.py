import sys, os
sys.path.insert(0, os.environ.get("GRAFT_REPO_ROOT", "/root/repo"))
import numpy as np, torch
from scarlet_amd import synth
from scarlet_amd.batch import BlendBatch
S = int(os.environ.get("STAMP_S", "10000"))
d = synth.make_batch(0, 512)
reps = (S + 511) // 512
imgs = np.tile(d["images"], (reps, 1, 1, 1))[:S]; cen = np.tile(d["centers"], (reps, 1, 1))[:S]
kw = {}
if len(sys.argv) > 1 and sys.argv[1] == "nocons": kw = dict(symmetric=False, monotonic=False)
b = BlendBatch(imgs, cen, **kw)
b.init_extended(np.ones(5) * .1)
b.fit(int(os.environ.get("STAMP_PRE", "3")), e_rel=0, check_every=0)
torch.cuda.synchronize()
PAIRS = bool(os.environ.get("STAMP_PAIRS"))     # library built with -DSC_STAMP_PAIRS: 8 more words per scene behind the stamps
b.workspace[:S * (24 if PAIRS else 16) * 8].zero_()
# STAMP_ITERS > 1: the multi-iteration kernel (k_fit2x); the stamps are those of the launch's LAST iteration
b.fit(int(os.environ.get("STAMP_ITERS", "1")), e_rel=0, check_every=0)
torch.cuda.synchronize()
st = b.workspace[:S * 16 * 8].view(torch.int64).view(S, 16).cpu().numpy()
pw_raw = None
if PAIRS:
    # per component: the lead's arrival at B5, and {arrival - B4, B4 - B3, last sweep level, NTR, NTC, slot} (fused2.h)
    pw = b.workspace[S * 16 * 8:S * 24 * 8].view(torch.int64).view(S, 4, 2).cpu().numpy()
    pw_raw = pw[:, :, 1]                                        # (every scene's words, in the stamps' order: STAMP_SYM)
    if int(os.environ.get("STAMP_ITERS", "1")) > 1 and S > 2048: pw = pw[:S - 1024]
    pw = pw[(pw[:, :, 0] > 0).all(axis=1)]                      # scenes with four present components
    arr, w = pw[:, :, 0].astype(np.float64), pw[:, :, 1]
    tail, sweep, lstop = w & 0xfffff, (w >> 20) & 0xfffff, (w >> 40) & 0xff
    ntr, ntc, slot = (w >> 48) & 7, (w >> 51) & 7, (w >> 54) & 3
    cost = ntr * ntc * (ntr + ntc)
    last = arr.argmax(axis=1)
    rows = np.arange(len(arr))
    print("B5 arrivals (n=%d scene-iterations): last - mean %d (p90 %d)   last - first %d (p90 %d)" % (
        len(arr), (arr.max(1) - arr.mean(1)).mean(), np.percentile(arr.max(1) - arr.mean(1), 90),
        (arr.max(1) - arr.min(1)).mean(), np.percentile(arr.max(1) - arr.min(1), 90)))
    print("   the last one: has the scene's largest GEMM cost in %.1f %%, its deepest sweep in %.1f %%; on slot 0/1/2/3 in %s %%" % (
        100.0 * (cost[rows, last] == cost.max(1)).mean(), 100.0 * (lstop[rows, last] == lstop.max(1)).mean(),
        np.round(100.0 * np.bincount(slot[rows, last], minlength=4) / len(arr), 1)))
    print("   (NTR, NTC) of the last one: share of scene-iterations, its lead's mean B3->B4 (sweep), last level, B4->B5")
    for a_, b_ in sorted(set(zip(ntr[rows, last].tolist(), ntc[rows, last].tolist()))):
        m = (ntr[rows, last] == a_) & (ntc[rows, last] == b_)
        print("      (%d, %d): %5.1f %%   sweep %6d   level %5.1f   tail %6d" % (a_, b_, 100.0 * m.mean(), sweep[rows, last][m].mean(),
              lstop[rows, last][m].mean(), tail[rows, last][m].mean()))
    lv = np.maximum(lstop, 1)
    print("   all leads: sweep %d cycles, %.0f per level; B4->B5 %d;  SIMDs {0,1} pairs' cost sum %.1f, SIMDs {2,3} %.1f" % (
        sweep.mean(), (sweep / lv).mean(), tail.mean(),
        np.where((slot & 1) == 0, cost, 0).sum(1).mean(), np.where((slot & 1) == 1, cost, 0).sum(1).mean()))
if int(os.environ.get("STAMP_ITERS", "1")) > 1 and S > 2048:
    # multi-iteration launch: the last iteration of the scenes that finish while the chip is still full (the last
    # ~1000 scenes of the queue finish beside emptying CUs and run faster)
    st = st[:S - 1024]
dt = np.diff(st[:, :7], axis=1)
if st[:, 10].any():
    print("P2 wave0: pre-sym %d  sym %d  sweep %d  tail %d" % ((st[:, 8] - st[:, 4]).mean(), (st[:, 9] - st[:, 8]).mean(),
          (st[:, 10] - st[:, 9]).mean(), (st[:, 5] - st[:, 10]).mean()))
if os.environ.get("STAMP_PROLOGUE"):
    # library built with -DSC_STAMP_PROLOGUE: slots 12 / 13 / 14 = wave 0 after its SED staging, after the iteration's
    # first barrier, in front of the gradient pass's first use of an image register (fused2.h)
    parts = [("start -> SED staged", st[:, 12] - st[:, 0]), ("-> past the first barrier", st[:, 13] - st[:, 12]),
             ("-> Gram stored, second barrier (stamp 1)", st[:, 1] - st[:, 13]), ("Lipschitz phase (stamp 1 -> 2)", st[:, 2] - st[:, 1]),
             ("stamp 2 -> first use of an image", st[:, 14] - st[:, 2]), ("first use of an image -> end of the gradient pass (stamp 3)", st[:, 3] - st[:, 14])]
    for name, v in parts:
        print("prologue: %-62s mean %6d  p50 %6d  p90 %6d" % (name, v.mean(), np.median(v), np.percentile(v, 90)))
elif os.environ.get("STAMP_SYM"):
    # library built with -DSC_STAMP_SYM (and -DSC_STAMP_PAIRS for the window's tile counts): slots 11 / 14 / 15 / 7 = wave 0
    # in front of its column sums, behind pair_ks_z, behind GEMM 1, behind GEMM 2 (fused2.h); wave 0 leads slot 0's pair
    ks = (st[:, 11] > 0) & (st[:, 14] > 0) & (st[:, 15] > 0) & (st[:, 7] > 0)          # k-space symmetry, not flip / centred
    sets = [("all leads", ks)]
    if pw_raw is not None:
        w = pw_raw[:len(st)]
        first = ((w >> 54) & 3) == 0
        ntr, ntc = (np.where(first, (w >> 48) & 7, 0)).max(1), (np.where(first, (w >> 51) & 7, 0)).max(1)
        sets.append(("4 x 4 tiles", ks & (ntr == 4) & (ntc == 4)))
    parts = [("colsums", 11, 8), ("wait B1", 8, 12), ("z", 12, 14), ("GEMM 1", 14, 15), ("wait B2", 15, 13), ("GEMM 2", 13, 7),
             ("wait B3", 7, 9)]
    for name, m in sets:
        print("sym wave0, %s (n=%d): " % (name, m.sum()) + "  ".join("%s %d" % (n, (st[m, j] - st[m, i]).mean()) for n, i, j in parts))
elif os.environ.get("STAMP_WORKER"):
    # library built with -DSC_STAMP_WORKER: slots 12 / 13 = start / end of the worker's step-size work (fused2.h), on
    # the worker wave; 9 / 10 = wave 0 after B3 / after B4 (its pair's sweep lies between them)
    ok = st[:, 13] > st[:, 12]
    print("worker: starts %d after wave 0's B3, works %d (p90 %d), ends %d before wave 0's B4; %.1f %% end after it  (n=%d)" % (
          (st[ok, 12] - st[ok, 9]).mean(), (st[ok, 13] - st[ok, 12]).mean(), np.percentile(st[ok, 13] - st[ok, 12], 90),
          (st[ok, 10] - st[ok, 13]).mean(), 100.0 * (st[ok, 13] > st[ok, 10]).mean(), ok.sum()))
elif st[:, 12].any():
    ok = st[:, 12] > 0
    if st[:, 11].any():
        print("sym wave0: vectors %d  rank1 %d  gemm1 %d  gemm2 %d  (n=%d)" % ((st[ok, 12] - st[ok, 8]).mean(), (st[ok, 13] - st[ok, 12]).mean(),
              (st[ok, 14] - st[ok, 13]).mean(), (st[ok, 9] - st[ok, 14]).mean(), ok.sum()))
    else:
        print("sym (pair kernel): to B1 %d  B1->B2 (rank1 z + gemm1) %d  B2->B3 (gemm2 + epilogue) %d" % ((st[ok, 12] - st[ok, 8]).mean(),
              (st[ok, 13] - st[ok, 12]).mean(), (st[ok, 9] - st[ok, 13]).mean()))
        o2 = st[:, 15] > 0
        print("   wave0: z %d  gemm1 %d  wait-B2 %d  (n=%d)" % ((st[o2, 14] - st[o2, 12]).mean(), (st[o2, 15] - st[o2, 14]).mean(),
              (st[o2, 13] - st[o2, 15]).mean(), o2.sum()))
    if st[:, 11].any(): print("P2 wave0 own tail:", (st[:, 11] - st[:, 10]).mean().round(0))
print("phase cycles mean:", dt.mean(axis=0).round(0), " total", (st[:, 6] - st[:, 0]).mean())
print("phase cycles p90 :", np.percentile(dt, 90, axis=0).round(0))
if st[:, 7].any() and st[:, 11].any() and not os.environ.get("STAMP_SYM"):
    cyc, ticks = (st[:, 6] - st[:, 0]).astype(float), (st[:, 11] - st[:, 7]).astype(float)
    ok = ticks > 0
    print("in-kernel clock (shader cycles per 100 MHz tick x 100 MHz): median %.0f MHz, p10 %.0f, p90 %.0f" % (
        np.median(cyc[ok] / ticks[ok]) * 100, np.percentile(cyc[ok] / ticks[ok], 10) * 100, np.percentile(cyc[ok] / ticks[ok], 90) * 100))
