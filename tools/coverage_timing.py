"""Times RigAnalyzer's default run on the GPU: 20 distances x 100 000 directions, the 1800 x 900 equirect with timings
and one full-resolution camera map, over the 16-camera synthetic rig. Kernel times come from the context's stage timer
(`coverage`); one JSON line per pass and repeat. For information only: nothing is gated on these numbers.

Usage: python tools/coverage_timing.py [--cams 16] [--res 2048] [--repeat 3]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cams", type=int, default=16)
    ap.add_argument("--res", type=int, default=2048)
    ap.add_argument("--repeat", type=int, default=3)
    args = ap.parse_args()
    from facebook360_dep_amd import derp, synth

    cams = synth.make_rig(args.cams, args.res)["cameras"]
    g = derp.Derp(cams)
    print("device", g.device_name(), flush=True)
    g.profile_enable(True)
    units, distances = derp.rig_fibonacci_units(100000), derp.rig_coverage_distances(0.5)
    g.coverage_directions(units[:1000], distances, want_counts=False)  # warm
    passes = (
        ("directions", lambda: g.coverage_directions(units, distances, want_counts=False), len(units) * len(distances)),
        ("equirect+timing", lambda: g.coverage_equirect(5), 1800 * 900),
        ("equirect", lambda: g.coverage_equirect(5, timing=False), 1800 * 900),
        ("camera", lambda: g.coverage_camera(0), args.res * args.res),
        ("cross_section", lambda: g.coverage_cross_section(400), 400 * 400),
    )
    for name, call, points in passes:
        for rep in range(args.repeat):
            g.profile_reset()
            t0 = time.perf_counter()
            call()
            wall = time.perf_counter() - t0
            q = g.profile_query("coverage", 0)
            sees = points * args.cams
            print(json.dumps(dict(kernel="k_coverage " + name, repeat=rep, cameras=args.cams, points=points,
                                  kernel_ms=round(q["ms"], 3), launches=q["launches"], api_wall_s=round(wall, 4), sees=sees,
                                  sees_per_s=round(sees / max(q["ms"] * 1e-3, 1e-9), 1))), flush=True)
    g.close()


if __name__ == "__main__":
    main()
