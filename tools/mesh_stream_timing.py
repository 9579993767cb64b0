"""Times and scores the mesh-stream renderer (derp_stream_*) on a synthetic rig through the binding, for DESIGN section
8.11. Nothing is gated on these numbers.

Scene: synth.make_rig(--cameras, --size), every camera's colour (8 bits) and true disparity; per camera the mesh
ConvertToBinary would write (derp_mesh_build + a simplifier + derp_mesh_download with the FLT_MIN clamp) for each of
  sequential  derp_mesh_simplify to --triangles (the reference's collapse loop, host)
  parallel    derp_mesh_simplify_parallel to --triangles (device)
  full        no simplifier (the budget is above the face count)
Views: cube faces of --edge pixels and a --snap snapshot, from the rig centre and from --offset metres off it.
Per variant and view one JSON line: derp_stream_render's wall time (uploads excluded, device synchronised, median of
--repeat after a warm call), derp_render's time for the same view from the full-resolution disparity (a yardstick: another
renderer, one vertex per pixel), and for the cube views the PSNR of the stream's picture against derp_render's (both as
8-bit sRGB codes, over the pixels both cover) with the share of pixels the stream leaves uncovered that derp_render covers.
--profile: per variant one derp_stream_render and one derp_render per view and nothing else, for a run under
rocprofv3 --kernel-trace --stats --output-format csv; --split TRACE.csv then reads that run's kernel trace and prints per
view the summed kernel time of the vertex stage, the two raster kernels, resolve and finish, and of derp_render's kernels
(the views are told apart by counting k_stream_finish / k_smr_finish: six per cube, one per snapshot).
--bin DIR --frames N: also writes the `--variant` meshes as an unfused <bin> tree of N (identical) frames with its rig.

Usage: python tools/mesh_stream_timing.py [--cameras 16] [--size 2048] [--triangles 150000] [--edge 2048] [--snap 3072x1536]
       [--offset 0.2] [--repeat 3] [--variants sequential,parallel,full] [--profile] [--bin DIR --frames 8 --variant parallel]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cameras", type=int, default=16)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--triangles", type=int, default=150000)
    ap.add_argument("--edge", type=int, default=2048)
    ap.add_argument("--snap", default="3072x1536")
    ap.add_argument("--offset", type=float, default=0.2)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--variants", default="sequential,parallel,full")
    ap.add_argument("--sequential_limit", type=float, default=20.0, help="seconds the first camera's sequential simplifier may take")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--split", default="")
    ap.add_argument("--bin", default="")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--variant", default="parallel")
    args = ap.parse_args()
    if args.split:
        return split(args.split, args.variants.split(","))
    from facebook360_dep_amd import derp, meshstream, synth

    rig = synth.make_rig(args.cameras, args.size)
    cams = rig["cameras"]
    g = derp.Derp(cams)
    print(json.dumps(dict(device=g.device_name(), cameras=args.cameras, size=args.size)), flush=True)
    colors, disps = [], []
    for cam in cams:
        bgr, disp, _, _ = synth.render_camera(cam, args.size, args.size)
        colors.append((bgr >> 8).astype(np.uint8))
        disps.append(disp.astype(np.float32))
    rgba = [np.ascontiguousarray(np.concatenate([c[..., ::-1], np.full(c.shape[:2] + (1,), 255, np.uint8)], axis=2)) for c in colors]
    table = derp.stream_srgb_table()

    def meshes(variant):
        out = []
        for s in range(len(cams)):
            t0 = time.perf_counter()
            _, faces, _ = g.mesh_build(s, disps[s])
            if variant == "sequential":
                g.mesh_simplify(args.triangles)
            elif variant == "parallel":
                g.mesh_simplify_parallel(args.triangles)
            out.append(g.mesh_download(clamp_negative_z=variant != "full"))
            seconds = time.perf_counter() - t0
            if s == 0:
                print(json.dumps(dict(variant=variant, camera0_faces_in=faces, camera0_faces_out=len(out[0][1]),
                                      camera0_mesh_seconds=round(seconds, 3))), flush=True)
                if variant == "sequential" and seconds > args.sequential_limit:
                    return None
            else:
                print(json.dumps(dict(variant=variant, camera=s, faces_out=len(out[s][1]), mesh_seconds=round(seconds, 3))), flush=True)
        return out

    w, h = (int(v) for v in args.snap.split("x"))
    off = (args.offset, 0.0, 0.0)
    views = [("cube", dict(kind="cube", height=args.edge), (0, 0, 0)), ("cube", dict(kind="cube", height=args.edge), off),
             ("snapshot", dict(kind="snapshot", width=w, height=h), (0, 0, 0)), ("snapshot", dict(kind="snapshot", width=w, height=h), off)]

    def timed(call):
        call()  # warm: code objects, buffers
        times = []
        for _ in range(max(1, args.repeat)):
            t0 = time.perf_counter()
            out = call()
            times.append(time.perf_counter() - t0)
        return out, sorted(times)[len(times) // 2]

    def codes_of_smr(img):
        with np.errstate(invalid="ignore"):
            return np.where(np.isnan(img), 0, np.clip(np.rint(img * 255), 0, 255)).astype(np.uint8)

    yard = {}
    g.render_upload(disps, [np.concatenate([c.astype(np.float32) / np.float32(255), np.ones(c.shape[:2] + (1,), np.float32)], axis=2)
                            for c in colors])
    for k, (name, kw, pos) in enumerate(views):
        if not args.profile:
            yard[k] = timed(lambda: g.render(derp.render_params(position=pos, **kw)))
    for variant in args.variants.split(","):
        scene = meshes(variant)
        if scene is None:
            print(json.dumps(dict(variant=variant, skipped="the sequential simplifier exceeded --sequential_limit on camera 0")), flush=True)
            continue
        t0 = time.perf_counter()
        for s, (vtx, idx) in enumerate(scene):
            g.stream_upload(s, vtx, idx, rgba[s])
        upload = time.perf_counter() - t0
        triangles = sum(len(idx) for _, idx in scene)
        for k, (name, kw, pos) in enumerate(views):
            p = derp.render_params(position=pos, **kw)
            if args.profile:
                g.stream_render(p)
                g.render(p)
                continue
            img, seconds = timed(lambda: g.stream_render(p))
            line = dict(variant=variant, view=name, position=pos, triangles=triangles, upload_seconds=round(upload, 3),
                        stream_render_ms=round(seconds * 1e3, 2), derp_render_ms=round(yard[k][1] * 1e3, 2))
            if name == "cube":
                ref = yard[k][0]
                mine, theirs = ~np.isnan(img[..., 3]), ~np.isnan(ref[..., 3])
                both = mine & theirs
                a = meshstream.srgb_encode(img[..., :3], table).astype(np.float64)[both]
                b = codes_of_smr(ref[..., :3]).astype(np.float64)[both]
                mse = float(((a - b) ** 2).mean())
                line.update(psnr_db=round(10 * np.log10(255.0 ** 2 / mse), 2) if mse > 0 else None,
                            uncovered_share=round(float((theirs & ~mine).sum()) / max(1, int(theirs.sum())), 5),
                            covered_by_both=int(both.sum()))
            print(json.dumps(line), flush=True)
        if args.bin and variant == args.variant:
            os.makedirs(args.bin, exist_ok=True)
            with open(os.path.join(args.bin, "rig_fused.json"), "w") as f:
                json.dump(rig, f)
            for s, cam in enumerate(cams):
                os.makedirs(os.path.join(args.bin, cam["id"]), exist_ok=True)
                for n in range(args.frames):
                    stem = os.path.join(args.bin, cam["id"], "%06d" % n)
                    scene[s][0].tofile(stem + ".vtx")
                    scene[s][1].tofile(stem + ".idx")
                    rgba[s].tofile(stem + ".rgba")
    g.close()


def split(trace, variants):
    """per (variant, view) the kernel times of a --profile run, from its kernel trace"""
    import csv

    rows = list(csv.DictReader(open(trace)))
    col = lambda part: next(c for c in rows[0] if part in c.lower())  # noqa: E731
    name, start, end = col("kernel_name"), col("start"), col("end")
    rows.sort(key=lambda r: int(r[start]))
    finishes = [6, 6, 1, 1]
    labels = ["cube centre", "cube off", "snapshot centre", "snapshot off"]
    for family, finish in (("k_stream_", "k_stream_finish"), ("k_smr_", "k_smr_finish")):
        keep = [r for r in rows if family in r[name] and not any(x in r[name] for x in ("k_stream_texture", "k_smr_mesh", "k_smr_texture"))]
        at = 0
        for variant in variants:
            for view, count in enumerate(finishes):
                per, seen = {}, 0
                while at < len(keep) and seen < count:
                    r = keep[at]
                    kernel = r[name].split("(")[0].replace("void ", "").replace("derp::", "").strip()
                    per[kernel] = per.get(kernel, 0) + int(r[end]) - int(r[start])
                    seen += finish in r[name]
                    at += 1
                print(json.dumps(dict(variant=variant, view=labels[view], kernels_ms={k: round(v / 1e6, 3) for k, v in sorted(per.items())},
                                      total_ms=round(sum(per.values()) / 1e6, 3))), flush=True)


if __name__ == "__main__":
    main()
