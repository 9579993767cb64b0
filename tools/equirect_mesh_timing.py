"""Times CreateObjFromDisparityEquirect's stages through the binding on a synthetic equirect (mesh_ref.gpu_disparity at
the given size): build, set-up, the sequential simplifier (set-up on the device, collapse loop on the host), the
pass-parallel simplifier on the device, and the host-only simplifier on the same mesh, each to --faces faces at
--strictness. Wall clock around calls that end in a device synchronise; device memory is what the context holds after
each stage (its buffers only grow). One JSON line per stage. For information only: nothing is gated on these numbers
(DESIGN section 8.10).

Usage: python tools/equirect_mesh_timing.py [--width 2048] [--height 1024] [--faces 200000] [--strictness 0.8]
       [--skip sequential,host]   (--host_only: the host-only simplifier alone, no device)"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--faces", type=int, default=200000)
    ap.add_argument("--strictness", type=float, default=0.8)
    ap.add_argument("--skip", default="")
    ap.add_argument("--host_only", action="store_true")
    args = ap.parse_args()
    skip = set(filter(None, args.skip.split(",")))
    from facebook360_dep_amd import derp, synth
    from tests import equirect_mesh_ref as E
    from tests import mesh_ref as R

    disp = R.gpu_disparity(args.width, args.height)

    def report(stage, seconds, **more):
        print(json.dumps(dict(stage=stage, width=args.width, height=args.height, seconds=round(seconds, 4), **more)), flush=True)

    def host_only(V, F):
        t0 = time.perf_counter()
        _, f, stats = derp.mesh_simplify_host(V, F, args.faces, args.strictness, False, False)
        report("host-only simplify (derp_mesh_simplify_host, set-up included)", time.perf_counter() - t0, faces=len(f), passes=stats[0])

    if args.host_only:
        m = E.build(disp) if args.width * args.height <= 1 << 16 else None
        assert m is not None, "--host_only builds the mesh in Python: keep it small, or run without it"
        host_only(m["V"], m["F"])
        return
    g = derp.Derp(synth.make_rig(1, 64)["cameras"])
    print("device", g.device_name(), flush=True)
    free0 = g.device_memory()[0]
    g.mesh_build_equirect(R.gpu_disparity(64, 32))  # warm: code objects
    g.mesh_setup(equi_error=False)

    def used():
        return round((free0 - g.device_memory()[0]) / 2 ** 20, 1)

    t0 = time.perf_counter()
    nv, nf, _ = g.mesh_build_equirect(disp)
    report("build", time.perf_counter() - t0, vertices=nv, faces=nf, device_mib=used())
    t0 = time.perf_counter()
    g.mesh_setup(equi_error=False)
    report("set-up (with its three downloads)", time.perf_counter() - t0, device_mib=used())
    V, F = g.mesh_download_f64()
    if "sequential" not in skip:
        t0 = time.perf_counter()
        stats = g.mesh_simplify(args.faces, args.strictness, equi_error=False)
        report("sequential simplify (device set-up, host loop)", time.perf_counter() - t0, faces=g.mesh_counts()[1], passes=stats[0],
               device_mib=used())
    if "parallel" not in skip:
        g.mesh_build_equirect(disp)
        t0 = time.perf_counter()
        stats = g.mesh_simplify_parallel(args.faces, args.strictness, equi_error=False)
        report("parallel simplify (device)", time.perf_counter() - t0, faces=g.mesh_counts()[1], passes=stats[0], device_mib=used())
    g.close()
    if "host" not in skip:
        host_only(V, F)


if __name__ == "__main__":
    main()
