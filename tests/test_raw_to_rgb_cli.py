"""The process boundary of bin/RawToRgb without a GPU: --helpxml against the flag table pinned from the reference's
source (tests/golden/ref_flags_raw_to_rgb.json, written by gen_ref_pins_isp.py with the reference's own get_flags
scraper), every refusal by message and exit status, the isp.json parser (cli/isp_config.h) through a small native
harness, and derp_isp_create without a device."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests.test_ref_pins import _cxx_literal, _helpxml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "facebook360_dep_amd")
BIN = os.path.join(PKG, "bin")


def test_flag_table_matches_the_reference(built):
    with open(os.path.join(ROOT, "tests", "golden", "ref_flags_raw_to_rgb.json")) as f:
        ref = json.load(f)["RawToRgb"]["flags"]
    mine = _helpxml("RawToRgb")
    assert len(ref) == 7
    type_of = {"string": "string", "integer": "int32", "boolean": "bool", "uint32": "uint32"}
    for fl in ref:
        name = fl["name"]
        got = mine[name]
        assert got["type"] == type_of[fl["type"]], name
        if fl["type"] == "string":
            assert got["default"] == _cxx_literal(fl["default"]), name
        elif fl["type"] == "boolean":
            assert (got["default"] == "true") == bool(fl["default"]), name
        elif fl["type"] == "uint32":
            # the scraped default is the expression static_cast<unsigned int>(DemosaicFilter::BILINEAR); BILINEAR is the
            # enum's first member, 0 (CameraIsp.h:32-38)
            assert "DemosaicFilter::BILINEAR" in fl["default"] and got["default"] == "0", name
        else:
            assert float(got["default"]) == float(fl["default"]), name
        assert got["meaning"] == _cxx_literal(fl["descr"]), (name, got["meaning"])
    names = {fl["name"] for fl in ref}
    for name, got in mine.items():
        assert name in names or "[extension" in got["meaning"] or got["meaning"].startswith("glog:"), name
    assert "[extension" in mine["device"]["meaning"] and "[extension" in mine["threads"]["meaning"]


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("raw_to_rgb")
    (root / "isp.json").write_text(json.dumps({"CameraIsp": {"width": 8, "height": 6, "bitsPerPixel": 16}}))
    (root / "000000.raw").write_bytes(bytes(8 * 6 * 2))
    (root / "short.raw").write_bytes(bytes(8 * 6 * 2 - 1))
    (root / "image.bin").write_bytes(bytes(8 * 6 * 2))
    (root / "odd").mkdir()
    (root / "odd" / "isp.json").write_text(json.dumps({"CameraIsp": {"width": 7, "height": 6}}))
    (root / "odd" / "000000.raw").write_bytes(bytes(7 * 6 * 2))
    (root / "deep").mkdir()
    (root / "deep" / "isp.json").write_text(json.dumps({"CameraIsp": {"width": 8, "height": 6, "bitsPerPixel": 12}}))
    (root / "deep" / "000000.raw").write_bytes(bytes(8 * 6 * 2))
    return root


def run(*args):
    p = subprocess.run([os.path.join(BIN, "RawToRgb")] + list(args), capture_output=True, text=True, timeout=60)
    return p.returncode, p.stderr


@pytest.mark.parametrize("args,message", [
    (["--input_image_path="], "input_image_path"),
    (["--demosaic_filter=1"], "frequency demosaic is not built"),
    (["--demosaic_filter=4"], "expecting Demosaic filter in [0,3]"),
    (["--demosaic_filter=-1"], "illegal value"),
    (["--output_dng_path=x.dng"], "dng output is not built"),
    (["--pow2_downscale_factor=3"], "expecting a resize value of 1, 2, 4, or 8. got 3"),
    (["--output_image_path="], "output_image_path"),
    (["--input_image_path={root}/image.bin"], ".raw"),
    (["--input_image_path={root}/image.bin", "--isp_config_path={root}/missing.json"], ".raw"),  # checked before the config
    (["--isp_config_path={root}/missing.json"], "could not read JSON file"),
    (["--input_image_path={root}/short.raw"], "unexpected end of file"),
    (["--input_image_path={root}/odd/000000.raw"], "must be even"),
    (["--input_image_path={root}/deep/000000.raw"], "Unsupported precision"),
    (["--input_image_path={root}/missing.raw"], "could not open raw image file"),
    (["--bogus_flag=1"], "bogus_flag"),
])
def test_refusals_need_no_device(built, tree, args, message):
    base = ["--input_image_path=%s/000000.raw" % tree, "--output_image_path=%s/out.png" % tree]
    rc, err = run(*(base + [a.format(root=tree) for a in args]))
    assert rc != 0 and message in err, (rc, err[-600:])
    assert "derp_isp_create" not in err  # refused before any device was asked for
    assert not (tree / "out.png").exists()


def test_directory_mode_refuses_a_short_file_before_any_device(built, tree, tmp_path):
    (tmp_path / "cam0").mkdir()
    (tmp_path / "cam0" / "000000.raw").write_bytes(bytes(8 * 6 * 2))
    (tmp_path / "cam0" / "short.raw").write_bytes(bytes(8 * 6 * 2 - 2))
    rc, err = run("--input_image_path=%s" % tmp_path, "--isp_config_path=%s/isp.json" % tree)
    assert rc != 0 and "unexpected end of file" in err and "short.raw" in err and "derp_isp_create" not in err


def test_isp_create_fails_loudly_without_a_device(built):
    import torch

    from facebook360_dep_amd import derp

    if torch.cuda.is_available():
        return
    with pytest.raises(derp.DerpError, match="no HIP device"):
        derp.Isp({"width": 8, "height": 6})
    for kwargs, message in ((dict(demosaic_filter=1), "frequency demosaic is not built"), (dict(demosaic_filter=7), "expecting Demosaic"),
                            (dict(pow2_downscale=5), "resize value")):
        with pytest.raises(derp.DerpError, match=message):  # refused before the device is looked for
            derp.Isp({"width": 8, "height": 6}, **kwargs)


# ---------------------------------------------------------------- cli/isp_config.h
@pytest.fixture(scope="module")
def harness(built, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("isp") / "isp_config_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", exe, os.path.join(ROOT, "tests", "native", "isp_config_main.cpp"), "-L" + PKG, "-lderp_hip",
                           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib", "-lz", "-ldl"])
    return exe


def parse(exe, tmp_path, text):
    path = tmp_path / "isp.json"
    path.write_text(text) if isinstance(text, str) else path.write_bytes(text)
    p = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=60)
    assert "AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-1500:]
    fields = {}
    for line in p.stdout.splitlines():
        k, _, v = line.partition(" ")
        fields.setdefault(k, []).append(v)
    return p, fields


F32 = lambda *v: " ".join("%.9g" % np.float32(x) for x in v)  # noqa: E731

DEFAULT_FIELDS = {
    "bitsPerPixel": ["16"], "width": ["0"], "height": ["0"], "isLittleEndian": ["0"], "isRowMajor": ["1"], "bayerPattern": ["GBRG"],
    "planeOrder": [""], "blackLevel": [F32(0, 0, 0)], "clampMin": [F32(0, 0, 0)], "clampMax": [F32(1, 1, 1)],
    "stuckPixelThreshold": ["0"], "stuckPixelDarknessThreshold": ["0"], "stuckPixelRadius": ["0"], "vignetteRollOffH": ["1"],
    "H": [F32(1, 1, 1)], "vignetteRollOffV": ["1"], "V": [F32(1, 1, 1)], "whiteBalanceGain": [F32(1, 1, 1)],
    "ccm": [F32(1, 0, 0, 0, 1, 0, 0, 0, 1)], "saturation": ["1"], "gamma": [F32(1, 1, 1)], "lowKeyBoost": [F32(0, 0, 0)],
    "highKeyBoost": [F32(0, 0, 0)], "contrast": ["1"], "sharpening": [F32(0, 0, 0)], "sharpeningSupport": [F32(10.0 / 2048.0)],
    "noiseCore": ["1000"], "compandingLut": ["2"],
}


def test_parser_defaults(harness, tmp_path):
    for text in ('{"CameraIsp": {}}', "{}", '{"other": 1}', '{"CameraIsp": null}', ' {\n"CameraIsp" : { "serial": 0, "name": "x" } }\n'):
        p, fields = parse(harness, tmp_path, text)
        assert p.returncode == 0 and fields == DEFAULT_FIELDS, (text, p.stderr[-300:], fields)


def test_parser_every_key(harness, tmp_path):
    cfg = {"bitsPerPixel": 8, "width": 640, "height": 480, "isLittleEndian": True, "isRowMajor": False, "bayerPattern": "rggb",
           "planeOrder": "gRbG", "compandingLut": [[0, 0, 0], [0.5, 0.6, 0.7], [1, 1, 1]], "blackLevel": [0.01, 0.02, 0.03],
           "clampMin": [0.1, 0.2, 0.3], "clampMax": [0.7, 0.8, 0.9], "stuckPixelThreshold": 5,
           "stuckPixelDarknessThreshold": 0.25, "stuckPixelRadius": 3, "vignetteRollOffH": [[1, 2, 3], [4, 5, 6]],
           "vignetteRollOffV": [[1.5, 1.25, 1.125], [0.5, 0.25, 0.125], [7, 8, 9]], "whiteBalanceGain": [1.1, 1.2, 1.3],
           "ccm": [[1.1, 0.2, 0.3], [0.4, 1.5, 0.6], [0.7, 0.8, 1.9]], "saturation": 1.3, "gamma": [0.4, 0.5, 0.6],
           "lowKeyBoost": [0.01, 0.02, 0.03], "highKeyBoost": [0.04, 0.05, 0.06], "contrast": 0.9, "sharpening": [0.1, 0.2, 0.3],
           "sharpeningSupport": 0.02, "noiseCore": 123.5}
    p, fields = parse(harness, tmp_path, json.dumps({"CameraIsp": cfg}))
    assert p.returncode == 0, p.stderr[-300:]
    want = {"bitsPerPixel": ["8"], "width": ["640"], "height": ["480"], "isLittleEndian": ["1"], "isRowMajor": ["0"],
            "bayerPattern": ["RGGB"], "planeOrder": ["GRBG"], "stuckPixelThreshold": ["5"], "stuckPixelRadius": ["3"],
            "stuckPixelDarknessThreshold": [F32(0.25)], "vignetteRollOffH": ["2"], "H": [F32(1, 2, 3), F32(4, 5, 6)],
            "vignetteRollOffV": ["3"], "V": [F32(1.5, 1.25, 1.125), F32(0.5, 0.25, 0.125), F32(7, 8, 9)],
            "ccm": [F32(*[v for row in cfg["ccm"] for v in row])], "saturation": [F32(1.3)], "contrast": [F32(0.9)],
            "sharpeningSupport": [F32(0.02)], "noiseCore": [F32(123.5)], "compandingLut": ["3"]}
    for k in ("blackLevel", "clampMin", "clampMax", "whiteBalanceGain", "gamma", "lowKeyBoost", "highKeyBoost", "sharpening"):
        want[k] = [F32(*cfg[k])]
    assert fields == want
    # one key at a time over the defaults: nothing else moves
    p, fields = parse(harness, tmp_path, '{"CameraIsp": {"contrast": 2}}')
    assert fields == dict(DEFAULT_FIELDS, contrast=["2"])


@pytest.mark.parametrize("text,message", [
    ("", "could not read JSON file"),
    ('{"CameraIsp": {"width": 8, "hei', "parse error"),
    ('{"CameraIsp": {"width": 8,', "parse error"),
    ('{"CameraIsp": {"width": }}', "parse error"),
    ('{"CameraIsp": {"width": 8}} trailing', "must hold one object"),
    ("[1, 2]", "must hold one object"),
    ('{"CameraIsp": 3}', "must be an object"),
    ('{"CameraIsp": {"width": "8"}}', "'width' must be a number"),
    ('{"CameraIsp": {"blackLevel": [0, 0]}}', "'blackLevel' must be an array of three numbers"),
    ('{"CameraIsp": {"gamma": 1}}', "'gamma' must be an array of three numbers"),
    ('{"CameraIsp": {"ccm": [[1, 0, 0], [0, 1, 0]]}}', "'ccm' must be a 3 x 3 matrix"),
    ('{"CameraIsp": {"bayerPattern": "RGB"}}', "'bayerPattern' must be a string of four letters"),
    ('{"CameraIsp": {"planeOrder": 4}}', "'planeOrder' must be a string of four letters"),
    ('{"CameraIsp": {"isRowMajor": "yes"}}', "'isRowMajor' must be true or false"),
    ('{"CameraIsp": {"vignetteRollOffH": [[1, 1]]}}', "'vignetteRollOffH' must be an array of points"),
    ('{"CameraIsp": {"vignetteRollOffH": [%s]}}' % ", ".join(["[1, 1, 1]"] * 17), "at most 16 are supported"),
    ('{"CameraIsp": {"stuckPixelThreshold": -1}}', "stuckPixelThreshold"),
    ("[" * 100, "nesting deeper"),
    (b"\xff\xfe{\x00", "parse error"),
])
def test_parser_refuses_bad_files(harness, tmp_path, text, message):
    p, _ = parse(harness, tmp_path, text)
    assert p.returncode == 1 and message in p.stderr, (p.returncode, p.stderr[-300:])
