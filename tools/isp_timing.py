#!/usr/bin/env python
"""Measure bin/RawToRgb the way DESIGN 8.4 reports it: a capture of N seeded 2048 x 2048 16-bit raw files in nested
camera folders, for demosaic filters 0 and 2 with sharpening on and off:

  * disk to disk: the directory-mode run (PNG files written), wall clock, after one warm-up run; files per second
  * per kernel: a separate run under `rocprofv3 --kernel-trace --stats` (skipped with --no-profile), each kernel's mean
    time and the bytes its stage has to move (computed here from the shapes) over that time, against the HBM peak

usage: tools/isp_timing.py OUT_DIR [files] [threads] [--no-profile]      (needs a GPU; prints and writes OUT_DIR/isp_timing.json)"""
import csv
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
BIN = os.path.join(ROOT, "facebook360_dep_amd", "bin", "RawToRgb")
HBM_PEAK_GBS = 8000.0  # as bench.py
W = H = 2048
N = W * H


def stage_bytes(kernel, bits=16):
    """what a stage must read + write at least, in bytes, from the shapes (fp32 planes of N pixels)"""
    f = 4 * N
    return {
        "k_isp_load": N * bits // 8 + f, "k_isp_pixel": 2 * f, "k_isp_bilinear": 4 * f, "k_isp_green_bilinear": 2 * f,
        "k_isp_ea_gradient": 3 * f + N, "k_isp_ea_vote": 3 * f + N, "k_isp_chroma": 4 * f, "k_isp_color": 6 * f,
        "k_isp_iir_rows": 3 * 4 * f, "k_isp_iir_cols": 3 * 4 * f, "k_isp_sharpen": 9 * f, "k_isp_output": 3 * f + 3 * N * bits // 8,
    }.get(kernel)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_dir = os.path.abspath(args[0])
    files = int(args[1]) if len(args) > 1 else 16
    threads = args[2] if len(args) > 2 else "-1"
    os.makedirs(out_dir, exist_ok=True)
    root = tempfile.mkdtemp(prefix="isp_timing_")
    rng = np.random.default_rng(7)
    for k in range(files):
        d = os.path.join(root, "capture", "cam%d" % (k % 4))
        os.makedirs(d, exist_ok=True)
        rng.integers(0, 65536, N, dtype=np.uint16).astype(">u2").tofile(os.path.join(d, "%06d.raw" % (k // 4)))
    base = {"width": W, "height": H, "bitsPerPixel": 16, "gamma": [0.45, 0.45, 0.45], "whiteBalanceGain": [1.4, 1.0, 1.6]}
    result = {"files": files, "size": [W, H], "threads": threads, "runs": []}
    for filt in (0, 2):
        for sharpen in (False, True):
            cfg = dict(base, sharpening=[0.5, 0.5, 0.5] if sharpen else [0, 0, 0])
            isp = os.path.join(root, "isp_%d_%d.json" % (filt, sharpen))
            with open(isp, "w") as f:
                json.dump({"CameraIsp": cfg}, f)
            cmd = [BIN, "--input_image_path=" + os.path.join(root, "capture"), "--isp_config_path=" + isp,
                   "--demosaic_filter=%d" % filt, "--threads=" + threads]
            walls = []
            for rep in range(3):  # the first run warms the page cache and the code object; it is not reported
                t0 = time.time()
                subprocess.run(cmd, check=True, capture_output=True, timeout=600)
                walls.append(time.time() - t0)
            assert len(glob.glob(os.path.join(root, "capture", "*", "*.png"))) == files
            run = {"filter": filt, "sharpen": sharpen, "wall_s": [round(w, 3) for w in walls[1:]],
                   "files_per_s": round(files / min(walls[1:]), 2), "kernels": {}}
            if "--no-profile" not in sys.argv:
                prof = os.path.join(out_dir, "rocprof_f%d_s%d" % (filt, sharpen))
                shutil.rmtree(prof, ignore_errors=True)
                subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", prof, "--output-format", "csv", "--"] + cmd,
                               check=True, capture_output=True, timeout=900)
                for path in glob.glob(os.path.join(prof, "**", "*kernel_stats.csv"), recursive=True):
                    for row in csv.DictReader(open(path)):
                        m = re.search(r"k_isp_[a-z_]+", row["Name"])
                        if not m:
                            continue
                        name = m.group(0)
                        mean_us = float(row["AverageNs"]) / 1e3
                        k = run["kernels"].setdefault(name, {"calls": 0, "mean_us": 0.0})
                        k["calls"] += int(row["Calls"])
                        k["mean_us"] = round(max(k["mean_us"], mean_us), 2)  # (u8 / u16 instantiations share a name)
                        b = stage_bytes(name)
                        if b:
                            k["min_bytes"] = b
                            k["gb_per_s"] = round(b / mean_us / 1e3, 1)
                            k["hbm_frac"] = round(b / mean_us / 1e3 / HBM_PEAK_GBS, 3)
                run["gpu_us_per_file"] = round(sum(k["mean_us"] for k in run["kernels"].values()), 1)
            result["runs"].append(run)
            print(json.dumps(run))
    with open(os.path.join(out_dir, "isp_timing.json"), "w") as f:
        json.dump(result, f, indent=1)
    shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
