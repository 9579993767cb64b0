#!/usr/bin/env python
"""Developer tool: how the blocks of the random-proposal and ping-pong launches fill the XCDs. Needs a library built with
-DDERP_BLOCK_TRACE=1 as DERP_LIB: every block then records its start and end on the 100 MHz clock the XCDs share
(derp_kernels.h, block_trace_end). One frame of the bench rig is processed; for the launches of levels 0 and 1 this
prints, per XCD (block id & 7: consecutive block ids go round the eight XCDs):
  last end    when the XCD's last block ended, before the end of the launch (us, and % of the launch): what an XCD
              idles at the end because its share of the work was smaller — the spread BETWEEN the XCDs
  resident    mean number of resident blocks per CU between the XCD's first start and its last end (sum of the blocks'
              lifetimes / that time / 32 CUs; 16 = four waves per SIMD all the time): the vacancy INSIDE the busy time
and for the whole launch the resident blocks per CU in each tenth of its duration (where the drain shows).
usage: DERP_LIB=.../libderp_var_trace.so [DERP_XCD_BANDS=K] [DERP_COST_TILES_PER_BLOCK=N] python tools/block_trace.py [config]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from facebook360_dep_amd import derp, synth  # noqa: E402

TICK_US = 0.01  # 100 MHz
CUS_PER_XCD = 32

n, res, widths = synth.config(sys.argv[1] if len(sys.argv) > 1 else "cfg2")
rig = synth.make_rig(n, res)
sizes = synth.level_sizes(res, res, widths)
frame = synth.make_frame(rig, sizes, device="cuda")
g = derp.Derp(rig["cameras"])
g.set_pyramid(sizes, res, res)
g.upload_frame(frame)
g.process_pyramid()
g.synchronize()
print("# %s, %d cameras %d x %d; DERP_XCD_BANDS=%s DERP_COST_TILES_PER_BLOCK=%s" % (
    g.device_name(), n, res, res, os.environ.get("DERP_XCD_BANDS", "(rule)"), os.environ.get("DERP_COST_TILES_PER_BLOCK", "(rule)")))
for stage in ("random_proposals", "ping_pong"):
    for level in (0, 1):
        t = g.block_trace(stage, level).astype(np.int64)
        gy, gx, _ = t.shape
        start, end = t[:, :, 0], t[:, :, 1]
        t0, t1 = start.min(), end.max()
        span = float(t1 - t0)
        life = (end - start).astype(np.float64)
        print("%s level %d: grid %d x %d, launch %.1f us, block lifetime mean %.1f us (median %.1f, max %.1f)" % (
            stage, level, gx, gy, span * TICK_US, life.mean() * TICK_US, np.median(life) * TICK_US, life.max() * TICK_US))
        print("  xcd  last end before the launch's  resident blocks / CU   blocks")
        worst = 0.0
        for xcd in range(8):
            s, e, lf = start[:, xcd::8], end[:, xcd::8], life[:, xcd::8]
            early = float(t1 - e.max())
            worst = max(worst, early)
            busy = float(e.max() - s.min())
            print("  %3d  %10.1f us  %6.2f %%          %6.2f               %d" % (
                xcd, early * TICK_US, 100.0 * early / span, lf.sum() / busy / CUS_PER_XCD, s.size))
        print("  spread between XCDs (earliest finisher): %.2f %% of the launch; mean idle over the eight: %.2f %%" % (
            100.0 * worst / span, 100.0 * np.mean([float(t1 - end[:, x::8].max()) for x in range(8)]) / span))
        # resident blocks per CU over the launch, by tenths: lifetime overlapping each tenth / its length / 256 CUs
        edges = t0 + span * np.arange(11) / 10.0
        row = []
        for a, b in zip(edges[:-1], edges[1:]):
            ov = np.clip(np.minimum(end, b) - np.maximum(start, a), 0, None).sum()
            row.append(ov / (b - a) / (8 * CUS_PER_XCD))
        print("  resident blocks / CU by tenth of the launch: " + " ".join("%.2f" % v for v in row))
g.close()
