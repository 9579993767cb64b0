"""bin/PngToPfm (source/conversion/PngToPfm.cpp): cv_util::loadImage<float> of a PNG written as a PFM, byte for byte
against imageio.write_pfm of the restated floats (tests/equirect_mesh_ref.py load_float). Host only: no device."""
import os
import subprocess

import numpy as np
import pytest

from tests import equirect_mesh_ref as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "facebook360_dep_amd", "bin", "PngToPfm")


def run(*args):
    p = subprocess.run([EXE] + list(args), capture_output=True, text=True, timeout=120)
    return p.returncode, p.stderr


@pytest.mark.parametrize("kind", ["gray8", "gray16", "bgr8", "bgra16"])
def test_pfm_bytes(built, tmp_path, kind):
    from facebook360_dep_amd import imageio as dio

    rng = np.random.default_rng(21)
    deep = kind.endswith("16")
    shape = (29, 37) if kind.startswith("gray") else (29, 37, 4 if kind.startswith("bgra") else 3)
    img = rng.integers(0, 65536 if deep else 256, shape, dtype=np.uint16 if deep else np.uint8)
    img.reshape(-1)[:2] = [0, 65535 if deep else 255]  # both ends of the range
    png, pfm, want = str(tmp_path / "in.png"), str(tmp_path / "out.pfm"), str(tmp_path / "want.pfm")
    (dio.write_png16 if deep else dio.write_png8)(png, img)
    rc, err = run("--png=" + png, "--pfm=" + pfm)
    assert rc == 0, err[-600:]
    floats = E.load_float(img)
    assert floats.dtype == np.float32 and floats.shape == (29, 37)
    assert floats.min() >= 0 and floats.max() <= 1 and (img.ndim == 3 or floats.max() == 1)
    dio.write_pfm(want, floats)
    assert open(pfm, "rb").read() == open(want, "rb").read()
    assert np.array_equal(dio.read_pfm(pfm), floats)
    assert "derp_create" not in err


@pytest.mark.parametrize("args,message", [(["--png="], 'Check failed: F.s("png") != ""'), (["--pfm="], 'Check failed: F.s("pfm") != ""'), (["--bogus_flag=1"], "bogus_flag")])
def test_bad_input_exits_nonzero(built, tmp_path, args, message):
    pfm = str(tmp_path / "out.pfm")
    rc, err = run(*(["--png=" + str(tmp_path / "nosuch.png"), "--pfm=" + pfm] + args))
    assert rc != 0 and message in err, (rc, err[-600:])
    assert "failed to load image" not in err and not os.path.exists(pfm)


def test_missing_png_is_refused(built, tmp_path):
    pfm = str(tmp_path / "out.pfm")
    rc, err = run("--png=" + str(tmp_path / "nosuch.png"), "--pfm=" + pfm)
    assert rc != 0 and "failed to load image" in err and not os.path.exists(pfm)
