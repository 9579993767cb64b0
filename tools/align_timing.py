"""Time AlignColors on the BASELINE config-2 rig (16 cameras of 2048^2): k_align_maps per camera and k_align_colors per
frame of all cameras (kernel times from device events through derp_profile_query, after a warmed first launch), the
latter as effective bandwidth over its compulsory bytes (image in, image out, both maps) next to a device-to-device
copy moving the same number of bytes in the same process; then bin/AlignColors from disk to disk over eight frames with
its own split into decode, device and encode. The frames are synth renders; two distinct frames are rendered and the
other six are copies of them (the codecs' times depend on the content, not on the name).

Usage: python tools/align_timing.py [--config cfg2] [--repeat 5] [--frames 8] [--no_tool] [--threads -1]
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


def reference_rigs(cam):
    """three one-camera reference rigs with a few pixels of lateral chromatic aberration at the rim"""
    d = list(cam.get("distortion", [0.0, 0.0, 0.0]))
    red = dict(cam, id="ref", focal=[cam["focal"][0] * 1.002, -cam["focal"][0] * 1.002], distortion=[d[0] * 0.9] + d[1:])
    blue = dict(cam, id="ref", focal=[cam["focal"][0] * 0.998, -cam["focal"][0] * 0.998], distortion=[d[0] * 1.1] + d[1:])
    return red, dict(cam, id="ref"), blue


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg2")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--no_tool", action="store_true")
    ap.add_argument("--threads", type=int, default=-1)
    args = ap.parse_args()

    import numpy as np
    import torch

    from facebook360_dep_amd import derp, synth
    from facebook360_dep_amd import imageio as dio

    n, res, _ = synth.config(args.config)
    rig = synth.make_rig(n, res)
    cams = rig["cameras"]
    red, green, blue = reference_rigs(cams[0])
    t0 = time.perf_counter()
    frames = [[synth.render_camera(c, res, res, frame=f)[0] for c in cams] for f in range(min(2, args.frames))]
    print("rendered %d frames of %d cameras of %d^2 in %.1f s" % (len(frames), n, res, time.perf_counter() - t0), flush=True)
    g = derp.Derp(cams)
    print("device", g.device_name(), flush=True)
    g.profile_enable(True)
    g.align_setup([red], [green], [blue])  # warm
    for rep in range(args.repeat):
        g.profile_reset()
        g.align_setup([red], [green], [blue])
        q = g.profile_query("align_maps", 0)
        print(json.dumps(dict(kernel="k_align_maps", repeat=rep, cameras=n, size=res, launches=q["launches"],
                              kernel_ms_all_cameras=round(q["ms"], 3), kernel_ms_per_camera=round(q["ms"] / n, 4))), flush=True)
    r0, b0 = g.align_maps(0)
    px, py = np.meshgrid(np.arange(res) + 0.5, np.arange(res) + 0.5)
    shift = np.maximum(np.hypot(r0[..., 0] - px, r0[..., 1] - py).max(), np.hypot(b0[..., 0] - px, b0[..., 1] - py).max())
    print(json.dumps(dict(largest_shift_px=round(float(shift), 3))), flush=True)
    pixels = n * res * res
    compulsory = pixels * (6 + 6 + 16)  # BGR u16 in, BGR u16 out, two float2 maps
    out = g.align_frame(frames[0])  # warm
    assert all(np.array_equal(o[..., 1], im[..., 1]) for o, im in zip(out, frames[0]))
    # a device-to-device copy that moves the same bytes (half of them read, half written), on the same device and process
    src = torch.empty(compulsory // 2, dtype=torch.uint8, device="cuda").random_(0, 256)
    dst = torch.empty_like(src)
    dst.copy_(src)
    torch.cuda.synchronize()
    for rep in range(args.repeat):
        g.profile_reset()
        t0 = time.perf_counter()
        g.align_frame(frames[rep % len(frames)])
        wall = time.perf_counter() - t0
        q = g.profile_query("align_colors", 0)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        dst.copy_(src)
        b.record()
        torch.cuda.synchronize()
        copy_ms = a.elapsed_time(b)
        print(json.dumps(dict(kernel="k_align_colors", repeat=rep, cameras=n, size=res, launches=q["launches"],
                              kernel_ms=round(q["ms"], 4), compulsory_bytes=compulsory,
                              effective_gb_per_s=round(compulsory / (q["ms"] * 1e-3) / 1e9, 1), copy_ms=round(copy_ms, 4),
                              copy_gb_per_s=round(compulsory / (copy_ms * 1e-3) / 1e9, 1),
                              kernel_over_copy=round(q["ms"] / copy_ms, 3), api_wall_s_with_host_copies=round(wall, 3))), flush=True)
    g.close()
    del src, dst
    if args.no_tool:
        return
    root = tempfile.mkdtemp(prefix="align_timing_")
    try:
        t0 = time.perf_counter()
        for name, rig_cams in (("rig_calibrated", cams), ("rig_red", [red]), ("rig_green", [green]), ("rig_blue", [blue])):
            with open(os.path.join(root, name + ".json"), "w") as f:
                json.dump({"cameras": rig_cams}, f)
        for k, c in enumerate(cams):
            os.makedirs(os.path.join(root, "color", c["id"]))
            for f in range(len(frames)):
                dio.write_png16(os.path.join(root, "color", c["id"], "%06d.png" % f), frames[f][k])
            for f in range(len(frames), args.frames):
                shutil.copy(os.path.join(root, "color", c["id"], "%06d.png" % (f % len(frames))),
                            os.path.join(root, "color", c["id"], "%06d.png" % f))
        print("wrote the dataset in %.1f s" % (time.perf_counter() - t0), flush=True)
        for rep in range(2):
            outdir = os.path.join(root, "out")
            t0 = time.perf_counter()
            p = subprocess.run([os.path.join(BIN, "AlignColors"), "--color=" + os.path.join(root, "color"), "--output=" + outdir,
                                "--threads=%d" % args.threads, "--calibrated_rig=" + os.path.join(root, "rig_calibrated.json")] +
                               ["--%s=%s" % (k, os.path.join(root, k + ".json")) for k in ("rig_red", "rig_green", "rig_blue")],
                               capture_output=True, text=True)
            wall = time.perf_counter() - t0
            files = [os.path.join(d, f) for d, _, fs in os.walk(outdir) for f in fs]
            summary = [line.split("] ", 1)[1] for line in p.stderr.split("\n") if " frames x " in line]
            print(json.dumps(dict(tool="AlignColors", repeat=rep, rc=p.returncode, frames=args.frames, wall_s=round(wall, 2),
                                  files=len(files), bytes=sum(os.path.getsize(f) for f in files), tool_says=summary)), flush=True)
            if p.returncode != 0:
                print(p.stderr[-1500:], flush=True)
                break
            shutil.rmtree(outdir, ignore_errors=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
