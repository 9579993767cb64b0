"""The RCCL halo exchange on REAL devices (TemporalBilateralFilter.cpp:96-184 / pipeline.py:364-408: the one
cross-frame data movement of the path). Every box this repo has seen so far has one GPU, where RCCL refuses a
second rank ("duplicate GPU") — so these tests skip there and run, unchanged, the moment `pytest -m gpu` lands on
a node with two or more devices: (a) the transport's self-test on 2 ranks / 2 devices, (b) the 5-frame `tiny`
sequence on 2 devices over ncclSend / ncclRecv == the 1-rank oracle run bit for bit with bytes = the plan's,
(c) `bin/DerpSequence --gpus 2 --exchange=rccl` byte-identical to one process, (d) `bench.py --gpus 2` as the
driver launches it: transport "rccl" on both ranks, result_crc == the CPU oracle's."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from tests import common

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIRST, LAST = 0, 4


def _device_count():
    try:
        import torch

        return torch.cuda.device_count()
    except Exception:  # noqa: BLE001
        return 0


needs_two = pytest.mark.skipif(_device_count() < 2, reason="needs >= 2 GPUs (RCCL refuses two ranks on one device)")


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rccl_worker(rank, world, port, out_dir):
    """One rank per process per device; the RCCL unique id travels over a gloo group (control plane only)."""
    import torch
    import torch.distributed as dist

    from facebook360_dep_amd import derp, sequence, synth

    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(rank)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    n, res, widths = synth.config("tiny")
    rig = synth.make_rig(n, res)
    sizes = synth.level_sizes(res, res, widths)
    g = derp.Derp(rig["cameras"], device=rank, partial_coverage=1)
    g.set_pyramid(sizes, res, res)
    r = sequence.SequenceRunner(g, FIRST, LAST, rank, world)
    for t in r.owned:
        r.upload_frame(t, synth.make_frame(rig, sizes, frame=t, seed=360 + t, device="cpu"))
    ident = [sequence.rccl_unique_id() if rank == 0 else None]
    dist.broadcast_object_list(ident, src=0)
    r.attach_rccl(ident[0])
    r.selftest(1 << 16)  # (a): a verified ring of ncclSend / ncclRecv on the library's stream
    r.exchange_inputs()
    r.run()
    g.synchronize()
    st = r.stats()
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), received=np.int64(st["bytes_received"]),
             **{"f%d_l%d" % (t, lv): np.stack([r.download_disparity(t, lv, d) for d in range(n)])
                for t in r.owned for lv in range(len(sizes))})
    r.close()
    g.close()
    dist.destroy_process_group()


@needs_two
def test_rccl_halo_exchange_on_two_devices(built, tmp_path):
    """(a) + (b): 2 ranks on 2 devices; every level of every frame equals the single-process CPU oracle run."""
    import torch.multiprocessing as mp

    from facebook360_dep_amd import sequence, synth

    world = 2
    mp.spawn(_rccl_worker, args=(world, _port(), str(tmp_path)), nprocs=world, join=True)
    n, res, widths = synth.config("tiny")
    rig = synth.make_rig(n, res)
    sizes = synth.level_sizes(res, res, widths)
    ref = common.OracleSequence(rig, sizes, res, FIRST, LAST, threads=-1)
    sequence.run_schedule(ref, list(range(len(sizes) - 1, -1, -1)), FIRST, LAST, 0, 1)
    received = 0
    for rank in range(world):
        z = np.load(os.path.join(str(tmp_path), "rank%d.npz" % rank))
        received += int(z["received"])
        for t in sequence.owned_frames(FIRST, LAST, world, rank):
            for lv in range(len(sizes)):
                assert common.bit_equal(z["f%d_l%d" % (t, lv)], ref.disp[t][lv].numpy()) == 0, (rank, t, lv)
    # bytes moved = the plan's: colour guides (8 B / texel as uploaded) once + raw level disparity at every level
    plan = sequence.plan(FIRST, LAST, world, 2, sequence.BLOCK)
    px = sum(w * h for (w, h) in sizes)
    assert received == len(plan) * px * n * (8 + 4)


@needs_two
def test_derp_sequence_two_gpus_over_rccl(built, tmp_path):
    """(c): the native multi-process program, one process per GPU, halo over RCCL: files equal one process's."""
    from facebook360_dep_amd import synth

    n, res, widths = synth.config("tiny")
    rig = synth.make_rig(n, res)
    sizes = synth.level_sizes(res, res, widths)
    root = str(tmp_path / "data")
    synth.write_dataset(root, rig, [0, 1, 2], sizes)
    exe = os.path.join(ROOT, "facebook360_dep_amd", "bin", "DerpSequence")
    flags = ["--input_root=" + root, "--first=000000", "--last=000002", "--partial_coverage", "--resolution=%d" % res]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    outs = {}
    for name, extra in (("one", []), ("two", ["--gpus=2", "--exchange=rccl"])):
        outs[name] = str(tmp_path / name)
        p = subprocess.run([exe] + flags + ["--output_root=" + outs[name]] + extra, capture_output=True, text=True,
                           timeout=900, env=env)
        assert p.returncode == 0, p.stderr[-3000:]
        if extra:
            assert "RCCL transport unavailable" not in p.stderr and "through files" not in p.stderr, p.stderr[-3000:]
    for kind in ("disparity_levels", "disparity_time_filtered_levels"):
        for level in range(len(sizes)):
            for cam in [c["id"] for c in rig["cameras"]]:
                for f in range(3):
                    rel = os.path.join(kind, "level_%d" % level, cam, "%06d.pfm" % f)
                    assert open(os.path.join(outs["two"], rel), "rb").read() == \
                        open(os.path.join(outs["one"], rel), "rb").read(), rel


@needs_two
def test_bench_two_gpus_over_rccl(built):
    """(d): the driver's N = 2 launch on two devices: both ranks report the RCCL transport and the depth maps
    (result_crc) are the CPU oracle's."""
    from facebook360_dep_amd import sequence, synth

    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(_port()), os.path.join(ROOT, "bench.py"),
                        "--full", "--gpus", "2", "--steps", "1", "--warmup", "1", "--config", "small", "--frames", "4",
                        "--synth-device", "cpu"], capture_output=True, text=True, timeout=900, cwd=ROOT,
                       env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"))
    assert p.returncode == 0, p.stderr[-3000:]
    out = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][0])
    assert out["n_gpus"] == 2 and out["halo_transport_per_rank"] == ["rccl", "rccl"], out["halo_transport_per_rank"]
    n, res, widths = synth.config("small")
    rig = synth.make_rig(n, res)
    sizes = synth.level_sizes(res, res, widths)
    seq = common.OracleSequence(rig, sizes, res, 0, 3, threads=-1, partial_coverage=False)
    sequence.run_schedule(seq, list(range(len(sizes) - 1, -1, -1)), 0, 3, 0, 1)
    assert out["result_crc"] == {str(t): "%08x" % v for t, v in seq.result_crc().items()}


@needs_two
def test_bench_plain_command_two_gpus(built):
    """(e): `python bench.py --gpus 2` with no launcher — what the driver's scaling run types — starts its own two
    ranks, one per device, over RCCL."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", "2", "--steps", "1",
                        "--warmup", "1", "--config", "small", "--frames", "4", "--synth-device", "cpu"], capture_output=True, text=True,
                       timeout=900, cwd=ROOT, env=dict(env, HSA_ENABLE_IPC_MODE_LEGACY="0"))
    assert p.returncode == 0, p.stderr[-3000:]
    out = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][0])
    assert out["n_gpus"] == 2 and out["halo_transport_per_rank"] == ["rccl", "rccl"], out["halo_transport_per_rank"]


def test_multi_device_tests_are_collected_and_skip_cleanly_on_one_gpu():
    """Keeps the file honest on a 1-GPU box: the gate is the device count, nothing else."""
    assert _device_count() >= 1
