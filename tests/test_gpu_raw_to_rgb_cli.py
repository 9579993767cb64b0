"""bin/RawToRgb end to end on small written captures: the PNGs decode to the image of tests/isp_ref.py (the CPU
restatement of the reference's ISP), in single-file mode and over a directory tree, whatever the number of I/O threads."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import isp_ref
from tests.test_gpu_isp import RICH, raw_bytes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "facebook360_dep_amd", "bin")


def run(*args):
    return subprocess.run([os.path.join(BIN, "RawToRgb")] + list(args), capture_output=True, text=True, timeout=120)


def listing(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, files in os.walk(root) for f in files)


@pytest.mark.parametrize("bits,filt,down", [(16, 0, 1), (8, 2, 1), (16, 3, 2)])
def test_single_file(built, tmp_path, bits, filt, down):
    from facebook360_dep_amd import imageio

    cfg = dict(RICH, width=70, height=38, bitsPerPixel=bits)
    raw = raw_bytes(cfg, 5)
    (tmp_path / "in").mkdir()
    (tmp_path / "in" / "isp.json").write_text(json.dumps({"CameraIsp": cfg}))  # found beside the input
    (tmp_path / "in" / "000000.raw").write_bytes(raw)
    out = tmp_path / "out.png"
    p = run("--input_image_path=%s" % (tmp_path / "in" / "000000.raw"), "--output_image_path=%s" % out,
            "--demosaic_filter=%d" % filt, "--pow2_downscale_factor=%d" % down)
    assert p.returncode == 0, p.stderr[-800:]
    want = isp_ref.Isp(cfg, filt, down).run(raw)["image"]
    got = imageio.read_png(str(out))
    assert got.dtype == want.dtype and np.array_equal(got, want)
    assert listing(tmp_path) == ["in/000000.raw", "in/isp.json", "out.png"]


def test_tone_curve_flag(built, tmp_path):
    from facebook360_dep_amd import imageio

    cfg = dict(RICH, width=70, height=38)
    raw = raw_bytes(cfg, 6)
    (tmp_path / "isp.json").write_text(json.dumps({"CameraIsp": cfg}))
    (tmp_path / "a.raw").write_bytes(raw)
    p = run("--input_image_path=%s" % (tmp_path / "a.raw"), "--output_image_path=%s" % (tmp_path / "a.png"),
            "--isp_config_path=%s" % (tmp_path / "isp.json"), "--apply_tone_curve=false")
    assert p.returncode == 0, p.stderr[-800:]
    assert np.array_equal(imageio.read_png(str(tmp_path / "a.png")), isp_ref.Isp(cfg, 0, 1, False).run(raw)["image"])


@pytest.fixture(scope="module")
def capture(tmp_path_factory):
    """a small tree: nested folders, 5 raw files, one bystander that is no .raw"""
    root = tmp_path_factory.mktemp("capture")
    # the raw stages stay at their defaults here: a clamp would tie values inside a stuck-pixel window
    cfg = {k: RICH[k] for k in ("ccm", "saturation", "gamma", "contrast", "sharpening", "sharpeningSupport", "noiseCore")}
    cfg.update(width=70, height=38, stuckPixelRadius=1, stuckPixelThreshold=1, stuckPixelDarknessThreshold=0.6)
    (root / "isp.json").write_text(json.dumps({"CameraIsp": cfg}))
    names = ["cam0/000000.raw", "cam0/000001.raw", "cam1/000000.raw", "cam1/more/deep/000007.raw", "top.raw"]
    want = {}
    ref = isp_ref.Isp(cfg, 2)
    for k, name in enumerate(names):
        os.makedirs(root / os.path.dirname(name), exist_ok=True)
        raw = raw_bytes(cfg, 10 + k)
        (root / name).write_bytes(raw)
        want[name[:-4] + ".png"] = ref.run(raw)["image"]
    (root / "cam0" / "notes.rawx").write_bytes(b"not a raw file")
    return dict(root=root, want=want, before=listing(root))


def test_directory_mode(built, capture, tmp_path):
    import shutil

    from facebook360_dep_amd import imageio

    files = {}
    for threads in (1, 4):
        root = tmp_path / ("threads%d" % threads)
        shutil.copytree(capture["root"], root)
        p = run("--input_image_path=%s" % root, "--isp_config_path=%s" % (root / "isp.json"), "--demosaic_filter=2",
                "--threads=%d" % threads)
        assert p.returncode == 0, p.stderr[-800:]
        assert listing(root) == sorted(capture["before"] + list(capture["want"]))  # every .raw got its .png, nothing else
        for name, want in capture["want"].items():
            assert np.array_equal(imageio.read_png(str(root / name)), want), name
        files[threads] = {name: (root / name).read_bytes() for name in capture["want"]}
    assert files[1] == files[4]  # byte-equal whatever the number of I/O threads
