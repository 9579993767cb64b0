#!/usr/bin/env python
"""Developer measurement (library built with -DDERP_COUNT_PP_FILL, through DERP_LIB): how full the ping-pong waves are
when they run computeCost. Per level: the cost evaluations computed (n_cost minus the memoised ones) against the lane-slots
the waves walked (64 per wave entry into computeCost; the fill build reports them in the pair-count slot).
DERP_PP_COMPACT=0 measures the one-pixel-per-lane candidate loop, the default the compacted one.
usage: DERP_LIB=.../libderp_var_fill.so python tools/pp_fill_probe.py [cfg2]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from facebook360_dep_amd import derp, synth  # noqa: E402

cfg = sys.argv[1] if len(sys.argv) > 1 else "cfg2"
n, res, widths = synth.config(cfg)
rig = synth.make_rig(n, res)
sizes = synth.level_sizes(res, res, widths)
g = derp.Derp(rig["cameras"], partial_coverage=int(n <= 4))
g.set_pyramid(sizes, res, res)
g.upload_frame(synth.make_frame(rig, sizes, frame=0, seed=360, device="cuda"))
g.profile_reset()
g.profile_enable(True)
g.process_pyramid()
g.synchronize()
print("%s, DERP_PP_COMPACT=%s" % (cfg, os.environ.get("DERP_PP_COMPACT", "1 (default)")))
for lv in range(len(sizes) - 1):
    q = g.profile_query("ping_pong", lv)
    memo = g.profile_memoised("ping_pong", lv)
    computed, slots = q["n_cost"] - memo, q["n_pair"]
    print("level %d: launches %d, evaluations %d (+ %d memoised), lane-slots walked %d, fill %.4f, ms %.2f" % (
        lv, q["launches"], computed, memo, slots, computed / max(slots, 1), q["ms"]))
g.close()
