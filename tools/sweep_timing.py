"""Time the rig preview tools on the BASELINE config-2 rig (16 cameras of 2048^2) at their defaults:
k_sweep_overlaps at --scale=0.5 with 50 depths for all 16 destinations, k_sweep_equirect at height 512 with 50 depths,
whole and cropped (kernel times from device events through derp_profile_query, after a warmed first launch), reported
as `sees` evaluations per second (pixels x depths x cameras, from the shapes), and each whole tool from disk to disk.

Usage: python tools/sweep_timing.py [--config cfg2] [--repeat 3] [--no_tools] [--threads -1]
Prints one JSON line per measurement."""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BIN = os.path.join(ROOT, "facebook360_dep_amd", "bin")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg2")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--no_tools", action="store_true")
    ap.add_argument("--threads", type=int, default=-1)
    args = ap.parse_args()

    import numpy as np

    from facebook360_dep_amd import derp, synth

    n, res, _ = synth.config(args.config)
    rig = synth.make_rig(n, res)
    cams = rig["cameras"]
    scale, num, height = 0.5, 50, 512
    small = int(np.floor(res * scale + 0.5))
    t0 = time.perf_counter()
    images = []
    for c in cams:  # rendered at the scaled size: the kernels' times do not depend on how the images were made
        bgr = synth.render_camera(c, small, small)[0].astype(np.float32) * (np.float32(1) / np.float32(65535))
        images.append(np.concatenate([bgr, np.ones(bgr.shape[:2] + (1,), np.float32)], axis=2))
    print("rendered %d cameras of %d^2 in %.1f s" % (n, small, time.perf_counter() - t0), flush=True)
    g = derp.Derp(cams)
    print("device", g.device_name(), flush=True)
    g.sweep_upload(images, [(res * scale, res * scale)] * n)
    g.profile_enable(True)
    disp = derp.sweep_overlap_disparities(num, 1, 10)[0]
    g.sweep_overlaps(0, disp[:2], u8=True)  # warm
    for rep in range(args.repeat):
        g.profile_reset()
        t0 = time.perf_counter()
        for d in range(n):
            g.sweep_overlaps(d, disp, u8=True)
        wall = time.perf_counter() - t0
        q = g.profile_query("sweep_overlaps", 0)
        sees = n * small * small * num * n
        print(json.dumps(dict(kernel="k_sweep_overlaps", repeat=rep, destinations=n, size=small, depths=num, kernel_ms=round(q["ms"], 3),
                              launches=q["launches"], api_wall_s=round(wall, 3), sees=sees,
                              sees_per_s=round(sees / (q["ms"] * 1e-3), 1))), flush=True)
    # the equirect at scale 1 (its default): the full-size images
    del images
    full = []
    for c in cams:
        bgr = synth.render_camera(c, res, res)[0].astype(np.float32) * (np.float32(1) / np.float32(65535))
        full.append(np.concatenate([bgr, np.ones(bgr.shape[:2] + (1,), np.float32)], axis=2))
    g.sweep_upload(full, [(float(res), float(res))] * n)
    depths = derp.sweep_equirect_depths(num, 1.0, 10.0)[0]
    W, H = 2 * height, height
    g.sweep_equirect(W, H, depths[:2], u8=True)  # warm
    for rep in range(args.repeat):
        g.profile_reset()
        g.sweep_equirect(W, H, depths, u8=True)
        q = g.profile_query("sweep_equirect", 0)
        sees = W * H * num * n
        print(json.dumps(dict(kernel="k_sweep_equirect", repeat=rep, size=[W, H], depths=num, kernel_ms=round(q["ms"], 3),
                              launches=q["launches"], sees=sees, sees_per_s=round(sees / (q["ms"] * 1e-3), 1))), flush=True)
    for rep in range(args.repeat):
        g.profile_reset()
        t0 = time.perf_counter()
        sees = 0
        for depth in depths:
            bounds = g.sweep_equirect_bounds(W, H, depth)
            new_w = derp.sweep_crop_size(H, bounds)
            g.sweep_equirect(W, H, [depth], window=bounds, out_size=(new_w, H), u8=True)
            sees += new_w * H * n
        wall = time.perf_counter() - t0
        q = g.profile_query("sweep_equirect", 0)
        print(json.dumps(dict(kernel="k_sweep_equirect cropped", repeat=rep, last_size=[new_w, H], depths=num,
                              kernel_ms=round(q["ms"], 3), launches=q["launches"], api_wall_s_with_bounds=round(wall, 3),
                              sees=sees, sees_per_s=round(sees / (q["ms"] * 1e-3), 1))), flush=True)
    g.close()
    if args.no_tools:
        return
    root = tempfile.mkdtemp(prefix="sweep_timing_")
    try:
        t0 = time.perf_counter()
        synth.write_dataset(root, rig, [0], [(res, res)])
        print("wrote the dataset in %.1f s" % (time.perf_counter() - t0), flush=True)
        base = ["--rig=" + os.path.join(root, "rigs", "rig_calibrated.json"),
                "--color=" + os.path.join(root, "video", "color_levels", "level_0"), "--threads=%d" % args.threads]
        for tool, extra in (("GenerateCameraOverlaps", []), ("GenerateEquirect", []), ("GenerateEquirect", ["--crop_equirect"]),
                            ("ProjectCamerasToEquirects", [])):
            out = os.path.join(root, "out_" + tool + "".join(extra).replace("--", "_"))
            t0 = time.perf_counter()
            p = subprocess.run([os.path.join(BIN, tool)] + base + ["--output=" + out] + extra, capture_output=True, text=True)
            wall = time.perf_counter() - t0
            files = [os.path.join(d, f) for d, _, fs in os.walk(out) for f in fs]
            print(json.dumps(dict(tool=tool, flags=extra, rc=p.returncode, wall_s=round(wall, 2), files=len(files),
                                  bytes=sum(os.path.getsize(f) for f in files))), flush=True)
            if p.returncode != 0:
                print(p.stderr[-1500:], flush=True)
                break
            shutil.rmtree(out, ignore_errors=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
