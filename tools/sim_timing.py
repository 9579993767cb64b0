#!/usr/bin/env python
"""Measure RigSimulator the way DESIGN 8.5 reports it (needs a GPU):

  * disk to disk: bin/RigSimulator --mode=rig_from_json on the 16-camera 2048 x 2048 rig, the default scene of 250
    icosahedra, --anti_alias_supersample=2 (PNG and PFM files written), wall clock, after one warm-up run
  * per kernel: a separate run under `rocprofv3 --kernel-trace --stats` (skipped with --no-profile): mean time per camera
    of the ray, trace and downscale kernels
  * CPU baseline: the same scene through derp_sim_trace_host (one thread, geometry only) on every 8th ray of camera 0
    in x and y, scaled to the camera's ray count
  * accuracy: a 256 x 256 capture of the same rig, cube scene in front of a textured skybox, run through the depth
    pipeline in process (derp.Derp: pyramid builder + every level, what bin/DerpCLI runs); per camera the median relative
    error of 1 / disparity against the simulator's true depth over the pixels that see geometry. Reported, not gated.

usage: tools/sim_timing.py OUT_DIR [--no-profile]      (prints and writes OUT_DIR/sim_timing.json)"""
import csv
import ctypes
import glob
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BIN = os.path.join(ROOT, "facebook360_dep_amd", "bin", "RigSimulator")
RES, AAS, CAMS = 2048, 2, 16


def textured_skybox(w=1024, h=512):
    rng = np.random.default_rng(11)
    coarse = rng.integers(0, 256, size=(h // 8, w // 8, 3), dtype=np.uint8)
    fine = rng.integers(-24, 25, size=(h, w, 3))
    return np.clip(np.kron(coarse, np.ones((8, 8, 1), dtype=np.int64)) + fine, 0, 255).astype(np.uint8)


def main():
    from facebook360_dep_amd import derp, imageio, synth

    out_dir = os.path.abspath([a for a in sys.argv[1:] if not a.startswith("--")][0])
    os.makedirs(out_dir, exist_ok=True)
    root = tempfile.mkdtemp(prefix="sim_timing_")
    sky = textured_skybox()
    imageio.write_png8(os.path.join(root, "sky.png"), sky)
    rig = synth.make_rig(CAMS, RES)
    with open(os.path.join(root, "rig.json"), "w") as f:
        json.dump(rig, f)
    result = {"cameras": CAMS, "size": [RES, RES], "aas": AAS, "scene": "250 icosahedra (default)"}

    # ---- disk to disk
    cmd = [BIN, "--mode=rig_from_json", "--rig_in=" + os.path.join(root, "rig.json"), "--skybox_path=" + os.path.join(root, "sky.png"),
           "--dest_cam_images=" + os.path.join(root, "images"), "--anti_alias_supersample=%d" % AAS]
    walls = []
    for rep in range(3):  # the first run warms the page cache and the code object; it is not reported
        t0 = time.time()
        subprocess.run(cmd, check=True, capture_output=True, timeout=600)
        walls.append(time.time() - t0)
    assert len(glob.glob(os.path.join(root, "images", "*"))) == 3 * CAMS
    result["disk_to_disk_s"] = [round(w, 3) for w in walls[1:]]
    print(json.dumps({"disk_to_disk_s": result["disk_to_disk_s"]}), flush=True)

    # ---- per kernel
    if "--no-profile" not in sys.argv:
        prof = os.path.join(out_dir, "rocprof_sim")
        shutil.rmtree(prof, ignore_errors=True)
        subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", prof, "--output-format", "csv", "--"] + cmd,
                       check=True, capture_output=True, timeout=900)
        kernels = {}
        for path in glob.glob(os.path.join(prof, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                m = re.search(r"k_sim_[a-z_]+|k_resize_area", row["Name"])
                if m:
                    k = kernels.setdefault(m.group(0), {"calls": 0, "total_ms": 0.0})
                    k["calls"] += int(row["Calls"])
                    k["total_ms"] += float(row["TotalDurationNs"]) / 1e6
        for k in kernels.values():
            k["ms_per_camera"] = round(k.pop("total_ms") / CAMS, 3)
        result["kernels"] = kernels
        shutil.rmtree(prof, ignore_errors=True)
        print(json.dumps({"kernels": kernels}), flush=True)

    # ---- CPU baseline: the process-start scene (srand(1) is the C library's state at the start of a process)
    ctypes.CDLL(None).srand(1)
    scene = derp.SimScene().icosahedrons(250).build_bvh()
    tris, nodes, leaf = scene.arrays()
    sim = derp.Sim()
    sim.upload(tris, nodes, leaf, sky)
    t0 = time.time()
    sim.render_camera(rig["cameras"][0], AAS)
    result["api_camera_ms"] = round((time.time() - t0) * 1e3, 2)  # one camera through the C-ABI, copies included
    o, d = sim.stage("origin")[::8, ::8], sim.stage("direction")[::8, ::8]
    rays = np.concatenate([o.reshape(-1, 3), d.reshape(-1, 3)], axis=1)
    t0 = time.time()
    scene.trace_host(rays)
    cpu = time.time() - t0
    result["cpu_single_thread_camera_ms"] = round(cpu * 64 * 1e3, 1)
    result["cpu_rays_traced"] = int(rays.shape[0])
    print(json.dumps({"cpu_single_thread_camera_ms": result["cpu_single_thread_camera_ms"]}), flush=True)

    # ---- accuracy against the true depth
    small = synth.make_rig(CAMS, 256)
    ctypes.CDLL(None).srand(1)
    cubes = derp.SimScene().cubes().build_bvh()
    sim.upload(*cubes.arrays(), sky)
    colors, depths = [], []
    for cam in small["cameras"]:
        bgr, depth = sim.render_camera(cam, AAS)
        colors.append(np.clip(np.rint(bgr), 0, 255).astype(np.uint16) * 257)
        depths.append(depth)
    sim.close()
    sizes = synth.level_sizes(256, 256, [256, 160, 100, 64])
    g = derp.Derp(small["cameras"])
    g.set_pyramid(sizes, 256, 256)
    for s, c in enumerate(colors):
        g.build_pyramid_color(s, c)
    g.process_pyramid()
    g.synchronize()
    acc = []
    for dcam in range(CAMS):
        disp = g.download_disparity(0, dcam)
        seen = np.isfinite(depths[dcam]) & (depths[dcam] < 1e30) & np.isfinite(disp) & (disp > 0)
        if seen.sum() == 0:
            acc.append({"camera": small["cameras"][dcam]["id"], "pixels": 0})
            continue
        rel = np.abs(1.0 / disp[seen] - depths[dcam][seen]) / depths[dcam][seen]
        acc.append({"camera": small["cameras"][dcam]["id"], "pixels": int(seen.sum()), "median_rel_depth_error": round(float(np.median(rel)), 4)})
    g.close()
    result["depth_accuracy_256"] = acc
    print(json.dumps({"depth_accuracy_256": acc}), flush=True)
    with open(os.path.join(out_dir, "sim_timing.json"), "w") as f:
        json.dump(result, f, indent=1)
    shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
