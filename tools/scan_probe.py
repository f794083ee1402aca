"""Phase timestamps inside k_gamma_scan<double,8> on the bench workload (debug build: make -C ideal-ballooning-solver_amd/csrc probe2 PM=8;
IBS_LIB_PATH=.../libibs_hip_probe2.so python tools/scan_probe.py).  One launch of the fused scan + argmax; per wave:
staging | set-up (incl. trial vector) | shift iteration (sweeps, decision code) | backward sweep | twisted | growth rate | epilogue,
and the hand-off of the surface maxima behind stamp 4 (16: after drain + block barrier, every wave; 17: the arrival add has returned,
wave 0; 18: end of the reduction, wave 0 of the blocks that complete a surface), printed for the block that finishes last."""
import os, sys, ctypes as C
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np, torch, ibs_amd, bench
from ibs_amd import _lib
dev = torch.device("cuda:0"); ctx = ibs_amd.Context(0)
h, geo7, dP_d, th0_d, base, dP, theta0 = bench.build_workload(0, dev)
plan = ibs_amd.ScanPlan(ctx, h, geo7, dP_d, th0_d, bench.N_SURF)
for _ in range(3): plan.scan_argmax()
torch.cuda.synchronize()
buf = np.zeros(1024 * 4 * (16 + 4), dtype=np.int64)          # 16-slot rows, then the 4-slot rows of the hand-off stamps (16 .. 19)
_lib.lib().ibs_probe_read(C.c_void_p(buf.ctypes.data), buf.size)
b = buf[:1024 * 4 * 16].reshape(1024, 4, 16)
ho = buf[1024 * 4 * 16:].reshape(1024, 4, 4)
ok = b[:, :, 0] > 0
w = b[ok]                                        # (waves, 16)
t0 = w[:, 0].min()
us = lambda x: x * 0.01
print("waves stamped: %d; kernel span (first start -> last end) %.2f us; start skew max %.2f us" % (len(w), us(w[:, 4].max() - t0), us(w[:, 0].max() - t0)))
twice = bool((w[:, 15] > 0).any())                 # (-DIBS_PROBE_TWICE build: the set-up ran twice, stamp 15 after the first)
names = [("staging + barrier", 0, 1)] + ([("set-up, FIRST execution", 1, 15), ("set-up, second: rows", 15, 8), ("set-up, second: sums", 8, 9)] if twice else
         [("set-up: row loop", 1, 8), ("set-up: bounds, trial sums", 8, 9)]) + [
         ("set-up + trial vector", 15 if twice else 1, 2), ("shift iteration", 2, 10), ("backward sweep", 10, 11),
         ("twisted + polish", 11, 12), ("growth: assemble, halo", 3, 13), ("growth: Simpson rows", 13, 14), ("growth: sums, division", 14, 4),
         ("growth rate", 3, 4), ("whole wave", 0, 4)]
for nm, a, c in names:
    d = us(w[:, c] - w[:, a])
    print("   %-24s median %6.2f  min %6.2f  max %6.2f us" % (nm, np.median(d), d.min(), d.max()))
nsw = w[:, 7]
print("   sweeps per solve: mean %.2f max %d; per sweep %.3f us; decision code per iteration %.3f us" % (
    nsw.mean(), nsw.max(), us(w[:, 5].sum()) / max(1, (nsw + 1).sum()), us(w[:, 6].sum()) / max(1, nsw.sum())))
end = us(w[:, 4] - t0)
print("   wave end times: median %.2f  p90 %.2f  max %.2f us" % (np.median(end), np.quantile(end, 0.9), end.max()))
slow = np.argsort(-end)[:5]
print("   slowest waves: end %s sweeps %s" % (np.round(end[slow], 2), nsw[slow]))
# ---- hand-off behind stamp 4: per block, from the block's last stamp 4 (its slowest wave has its growth rate)
t4 = np.where(ok, b[:, :, 4], 0).max(axis=1)                  # (blocks,)
t16 = ho[:, :, 0].max(axis=1); t17 = ho[:, 0, 1]; t18 = ho[:, 0, 2]
red = np.nonzero(t18 > t17)[0]                                # blocks that completed a surface in THIS launch (the stamps of earlier launches stay)
if len(red):
    seg = lambda x: us(x[red])
    print("   hand-off, the %d blocks that completed a surface (us, median / max): drain + barrier %.2f / %.2f | arrival add %.2f / %.2f | read back + reduce %.2f / %.2f | stamp 4 -> end %.2f / %.2f" % (
        len(red), np.median(seg(t16 - t4)), seg(t16 - t4).max(), np.median(seg(t17 - t16)), seg(t17 - t16).max(),
        np.median(seg(t18 - t17)), seg(t18 - t17).max(), np.median(seg(t18 - t4)), seg(t18 - t4).max()))
    k = red[np.argmax(t18[red])]
    print("   block that finishes last (block %d): last wave's growth rate at %.2f us | drain + barrier %.2f | arrival add %.2f | read back + reduce %.2f | ends %.2f us" % (
        k, us(t4[k] - t0), us(t16[k] - t4[k]), us(t17[k] - t16[k]), us(t18[k] - t17[k]), us(t18[k] - t0)))
    oth = np.setdiff1d(np.nonzero(t17 > 0)[0], red)
    if len(oth):
        print("   other blocks: drain + barrier median %.2f | arrival add median %.2f us" % (np.median(us(t16[oth] - t4[oth])), np.median(us(t17[oth] - t16[oth]))))
