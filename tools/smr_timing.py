#!/usr/bin/env python
"""SimpleMeshRenderer's cost on one GPU: write a synth dataset of a BASELINE config (colour + truth disparity, one
frame), then for every --format run bin/SimpleMeshRenderer from disk (wall time of the process: decode, upload,
render, encode, write; HIP start-up included) and once more under `rocprofv3 --kernel-trace --stats` (summed device
time of its kernels). For comparison, ComputeRephotographyErrors on the same frame (--cameras=cam0: two cubemaps of
edge = the image height) under rocprofv3: the canopy kernels' time per cubemap.
usage: tools/smr_timing.py [config=cfg2] [width=3072] [file_type=png]   (prints one JSON line per measurement)"""
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from facebook360_dep_amd import derp, synth  # noqa: E402
from tests import smr_dataset  # noqa: E402

BIN = os.path.join(ROOT, "facebook360_dep_amd", "bin")


def kernel_ns(cmd, tag, root):
    """summed TotalDurationNs per kernel of one rocprofv3 --kernel-trace --stats run of cmd"""
    out = os.path.join(root, "prof_" + tag)
    subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", tag, "--"] + cmd,
                   check=True, capture_output=True, timeout=900)
    per = {}
    for path in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            name = row["Name"].split("(")[0].replace("void ", "").replace("derp::", "").strip()
            per[name] = per.get(name, 0) + int(float(row["TotalDurationNs"]))
    return per


def main():
    cfg = sys.argv[1] if len(sys.argv) > 1 else "cfg2"
    width = int(sys.argv[2]) if len(sys.argv) > 2 else 3072
    ftype = sys.argv[3] if len(sys.argv) > 3 else "png"
    n, res, _ = synth.config(cfg)
    root = tempfile.mkdtemp(prefix="smr_timing_", dir="/tmp")
    t0 = time.time()
    smr_dataset.write(root, n=n, res=res, frames=(0,))
    print("dataset: %s (%d x %d^2) written in %.1f s" % (cfg, n, res, time.time() - t0), flush=True)
    base = [os.path.join(BIN, "SimpleMeshRenderer"), "--rig=" + os.path.join(root, "rig.json"),
            "--color=" + os.path.join(root, "color"), "--disparity=" + os.path.join(root, "disparity"),
            "--width=%d" % width, "--file_type=" + ftype]
    for fmt in derp.FORMATS:
        cmd = base + ["--format=" + fmt, "--output=" + os.path.join(root, "out_" + fmt)]
        t0 = time.time()
        subprocess.run(cmd, check=True, capture_output=True, timeout=900)
        wall = time.time() - t0
        per = kernel_ns(cmd, fmt, root)
        print(json.dumps({"config": cfg, "format": fmt, "width": width, "file_type": ftype, "disk_to_disk_s": round(wall, 3),
                          "kernel_ms": round(sum(per.values()) / 1e6, 2),
                          "render_kernel_ms": round(sum(v for k, v in per.items() if k.startswith("k_smr")) / 1e6, 2),
                          "top": sorted(((k, round(v / 1e6, 2)) for k, v in per.items()), key=lambda kv: -kv[1])[:4]}),
              flush=True)
    cmd = [os.path.join(BIN, "ComputeRephotographyErrors"), "--rig=" + os.path.join(root, "rig.json"),
           "--color=" + os.path.join(root, "color"), "--disparity=" + os.path.join(root, "disparity"), "--first=000000",
           "--last=000000", "--cameras=cam0", "--output=" + os.path.join(root, "out_rephoto")]
    per = kernel_ns(cmd, "rephoto", root)
    canopy = sum(v for k, v in per.items() if k.startswith("k_canopy"))
    print(json.dumps({"config": cfg, "ComputeRephotographyErrors": "cam0", "cubemaps": 2, "edge": res,
                      "canopy_kernel_ms_per_cubemap": round(canopy / 2e6, 2)}), flush=True)


if __name__ == "__main__":
    main()
