"""Time one frame of GeometricConsistency on the BASELINE config-2 rig (16 cameras of 2048^2) at the tool's defaults
(downscale 4, disparity_step 0.5, two passes): wall time of derp_gc_upload + derp_gc_run, the kernels' times from
derp_profile_query, and reprojections per second of the sweep (slices x sources x destination pixels, halo not counted).

Usage: python tools/geometric_timing.py [--config cfg2] [--downscale 4] [--disparity_step 0.5] [--pass_count 2] [--repeat 3]
Prints one JSON line per repeat (the first includes the allocations) and a summary line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg2")
    ap.add_argument("--downscale", type=float, default=4.0)
    ap.add_argument("--disparity_step", type=float, default=0.5)
    ap.add_argument("--agree_fraction", type=float, default=0.75)
    ap.add_argument("--pass_count", type=int, default=2)
    ap.add_argument("--repeat", type=int, default=3)
    args = ap.parse_args()

    import numpy as np

    from facebook360_dep_amd import derp, synth

    n, res, _ = synth.config(args.config)
    cams = synth.make_rig(n, res)["cameras"]
    t0 = time.perf_counter()
    images = [synth.render_camera(c, res, res)[0] for c in cams]
    print("rendered %d cameras of %d^2 in %.1f s" % (n, res, time.perf_counter() - t0), flush=True)
    sizes = [tuple(int(np.floor(r / args.downscale + 0.5)) for r in c["resolution"]) for c in cams]
    g = derp.Derp(cams)
    print("device", g.device_name(), flush=True)
    g.profile_enable(True)
    rows = []
    for rep in range(args.repeat):
        g.profile_reset()
        t0 = time.perf_counter()
        g.gc_upload(images, sizes)
        t1 = time.perf_counter()
        g.gc_run(args.disparity_step, args.agree_fraction, args.pass_count, False)
        g.synchronize()
        t2 = time.perf_counter()
        slices = [len(g.gc_slices(d, args.disparity_step)) for d in range(n)]
        sweeps = 1 + args.pass_count
        reprojections = sweeps * sum(slices[d] * (n - 1) * sizes[d][0] * sizes[d][1] for d in range(n))
        ms = {k: g.profile_query(k, 0) for k in ("gc_prepare", "gc_sweep", "gc_clean")}
        row = dict(repeat=rep, cameras=n, full=res, small=sizes[0], slices=slices[0], upload_wall_s=round(t1 - t0, 4),
                   run_wall_s=round(t2 - t1, 4), prepare_ms=round(ms["gc_prepare"]["ms"], 3),
                   sweep_ms=round(ms["gc_sweep"]["ms"], 3), sweep_launches=ms["gc_sweep"]["launches"],
                   clean_ms=round(ms["gc_clean"]["ms"], 3), reprojections=reprojections,
                   reprojections_per_s=round(reprojections / (ms["gc_sweep"]["ms"] * 1e-3), 1) if ms["gc_sweep"]["ms"] else None)
        rows.append(row)
        print(json.dumps(row), flush=True)
    best = min(rows, key=lambda r: r["run_wall_s"])
    depth = g.gc_result("depth", 0, args.pass_count - 1) if args.pass_count else g.gc_result("iffy", 0)
    print(json.dumps(dict(summary=True, best_run_wall_s=best["run_wall_s"], best_sweep_ms=min(r["sweep_ms"] for r in rows),
                          reprojections_per_s=max(r["reprojections_per_s"] or 0 for r in rows),
                          finite_share_cam0=round(float(np.isfinite(depth).mean()), 4))), flush=True)
    g.close()


if __name__ == "__main__":
    main()
