"""Reading the fused mesh stream back, without a GPU: facebook360_dep_amd/meshstream.py and cli/mesh_stream_io.h (through
the stand-alone program tests/native/mesh_stream_main.cpp, built with AddressSanitizer + UBSan and run directly; nothing
sanitized is loaded into Python) against ConvertToBinary's fusion of the hand-made tree of
tests/test_convert_to_binary_cli.py (file sizes 0, 1, 512 Ki, 512 Ki + 1; 1 and 3 strips); the legacy catalog, the
endianness check, ranges past the end of a strip file, truncated and garbage catalogs; the sRGB decode table and its
inverse."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests.test_convert_to_binary_cli import bin_tree, run as convert_to_binary  # noqa: F401  (bin_tree is a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mesh_stream") / "mesh_stream_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", exe, os.path.join(ROOT, "tests", "native", "mesh_stream_main.cpp"), "-lz", "-pthread"])
    return exe


def native(harness, *args):
    p = subprocess.run([harness] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert "AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-1500:]
    return p.returncode, p.stdout, p.stderr


@pytest.fixture(scope="module", params=[1, 3])
def fused(request, built, bin_tree, tmp_path_factory):
    root, cams, data = bin_tree
    out = str(tmp_path_factory.mktemp("fused%d" % request.param))
    rc, err = convert_to_binary("--rig=" + os.path.join(root, "rig.json"), "--bin=" + os.path.join(root, "bin"), "--fused=" + out,
                                "--first=000004", "--last=000005", "--output_formats=vtx,,idx", "--run_conversion=false",
                                "--fuse_strip=%d" % request.param, "--device=99")
    assert rc == 0, err[-800:]
    return out, [os.path.join(out, "fused_%d.bin" % i) for i in range(request.param)], data


def test_python_reader_reads_the_fusion_back(fused):
    from facebook360_dep_amd import meshstream

    out, strips, data = fused
    stream = meshstream.MeshStream(os.path.join(out, "fused.json"), strips)
    assert sorted(stream.catalog) == ["000004", "000005"]
    for (frame, cam, ext), blob in data.items():
        assert stream.read(frame, cam, ext) == blob, (frame, cam, ext, len(blob))
    with pytest.raises(meshstream.MeshStreamError, match="is missing from frame 000004"):
        stream.read("000004", "nosuchcam", ".vtx")
    with pytest.raises(meshstream.MeshStreamError, match="frame 000009 is not in the catalog"):
        stream.read("000009", "cam0", ".vtx")
    with pytest.raises(meshstream.MeshStreamError, match="holds no .rgba"):
        stream.read("000004", "cam0", ".rgba")


def test_native_reader_reads_the_fusion_back(fused, harness, tmp_path):
    out, strips, data = fused
    rc, text, err = native(harness, "catalog", os.path.join(out, "fused.json"))
    assert rc == 0, err[-500:]
    listed = {}
    for line in text.splitlines():
        frame, cam, ext, offset, size = line.split()
        listed[(frame, cam, ext)] = (int(offset), int(size))
    assert sorted(listed) == sorted(data)
    for key, blob in data.items():
        got = str(tmp_path / "got.bin")
        rc, _, err = native(harness, "read", listed[key][0], listed[key][1], got, *strips)
        assert rc == 0 and open(got, "rb").read() == blob, (key, err[-300:])


def test_ranges_past_the_end_are_refused(fused, harness, tmp_path):
    from facebook360_dep_amd import meshstream

    out, strips, _ = fused
    reader = meshstream.StripedReader(strips)
    total = sum(reader.lengths)
    stripe = meshstream.STRIPE
    for offset, size in ((total, 1), (0, total + 1), (total - 1, 2), (10 * total, 0 + 1), (2 ** 62, 2 ** 62), (stripe - 1, total)):
        with pytest.raises(meshstream.MeshStreamError, match="lie past the end of"):
            reader.read(offset, size)
        rc, _, err = native(harness, "read", offset, size, tmp_path / "x.bin", *strips)
        assert rc == 1 and "lie past the end of" in err, (offset, size, err[-300:])
    assert reader.read(total, 0) == b"" and len(reader.read(0, min(total, 3 * stripe))) == min(total, 3 * stripe)
    rc, _, err = native(harness, "read", 2 ** 64 - 1, 2, tmp_path / "x.bin", *strips)
    assert rc == 1 and "overflows" in err
    rc, _, err = native(harness, "read", 0, 1, tmp_path / "x.bin", str(tmp_path / "nosuch.bin"))
    assert rc == 1 and "cannot open strip file" in err
    with pytest.raises(meshstream.MeshStreamError, match="cannot open strip file"):
        meshstream.StripedReader([str(tmp_path / "nosuch.bin")])


def test_catalog_forms(harness, tmp_path):
    from facebook360_dep_amd import meshstream

    frames = {"000000": {"cam0": {".vtx": {"offset": 0, "size": 36}, ".idx": {"offset": 36, "size": 12}, "offset": 0, "size": 48}}}
    want = {"000000": {"cam0": {".vtx": (0, 36), ".idx": (36, 12)}}}

    def both(text, name):
        path = str(tmp_path / name)
        with open(path, "w") as f:
            f.write(text)
        rc, out, err = native(harness, "catalog", path)
        try:
            parsed = meshstream.parse_catalog(text)
        except meshstream.MeshStreamError as e:
            parsed = str(e)
        return rc, out, err, parsed

    for text in (json.dumps({"metadata": {"isLittleEndian": True}, "frames": frames}), json.dumps(frames)):  # current, legacy
        rc, out, err, parsed = both(text, "ok.json")
        assert rc == 0 and parsed == want, err[-300:]
        assert sorted(out.splitlines()) == ["000000 cam0 .idx 36 12", "000000 cam0 .vtx 0 36"]
    rc, _, err, parsed = both(json.dumps({"metadata": {"isLittleEndian": False}, "frames": frames}), "big.json")
    assert rc == 1 and "Endianness mismatch" in err and "Endianness mismatch" in parsed
    good = json.dumps({"metadata": {"isLittleEndian": True}, "frames": frames})
    bad = {
        "empty": "", "truncated": good[:len(good) // 2], "one_brace": "{", "garbage": "\x00\xff\x7f{]]\"", "array": "[1, 2, 3]",
        "legacy_with_frames": json.dumps({"frames": frames}), "no_frames": json.dumps({"metadata": {"isLittleEndian": True}}),
        "frames_is_a_list": json.dumps({"metadata": {"isLittleEndian": True}, "frames": [1]}),
        "negative": good.replace('"offset": 36', '"offset": -36'), "fraction": good.replace('"size": 12', '"size": 12.5'),
        "text": good.replace('"size": 12', '"size": "12"'), "deep": "[" * 100000,
        "endianness_is_a_number": good.replace("true", "1"),
    }
    for name, text in bad.items():
        rc, _, err, parsed = both(text, name + ".json")
        assert rc == 1 and isinstance(parsed, str), (name, rc, parsed, err[-300:])


def test_renderer_inputs_of_a_camera(harness, tmp_path):
    from facebook360_dep_amd import meshstream

    def entry(*exts):
        return {e: {"offset": 0, "size": 0} for e in exts}

    frames = {"000000": {"ok": entry(".vtx", ".idx", ".rgba", ".bc7"), "bc7": entry(".vtx", ".idx", ".bc7"), "bare": entry(".vtx", ".idx")}}
    path = str(tmp_path / "fused.json")
    with open(path, "w") as f:
        json.dump({"metadata": {"isLittleEndian": True}, "frames": frames}, f)
    strip = str(tmp_path / "fused_0.bin")
    open(strip, "wb").close()
    stream = meshstream.MeshStream(path, [strip])
    assert native(harness, "camera", path, "000000", "ok")[0] == 0 and stream.read("000000", "ok", ".rgba") == b""
    for cam, message in (("bc7", "bc7 colour is not built; write the stream with --output_formats=idx,vtx,rgba"),
                         ("bare", "holds no .rgba"), ("gone", "camera gone of the rig is missing from frame 000000")):
        rc, _, err = native(harness, "camera", path, "000000", cam)
        assert rc == 1 and message in err, err[-300:]
        with pytest.raises(meshstream.MeshStreamError, match=message):
            stream.read("000000", cam, ".rgba")


def test_srgb_table_and_its_inverse(built, harness, tmp_path):
    from facebook360_dep_amd import derp, meshstream

    table = derp.stream_srgb_table()
    s = np.arange(256) / 255.0
    ref = np.where(s <= 0.04045, s / 12.92, ((s + 0.055) / 1.055) ** 2.4).astype(np.float32)
    assert np.abs(table.view(np.int32).astype(np.int64) - ref.view(np.int32)).max() <= 1  # one float ulp
    assert table[0] == 0 and table[255] == 1 and (np.diff(table) > 0).all()
    assert np.array_equal(meshstream.srgb_encode(table, table), np.arange(256))  # encode o decode = identity
    mid = ((table[:-1].astype(np.float64) + table[1:]) / 2).astype(np.float32)
    exact = mid.astype(np.float64) == (table[:-1].astype(np.float64) + table[1:]) / 2
    assert np.array_equal(meshstream.srgb_encode(mid, table)[exact], np.arange(255)[exact])  # ties go to the lower code
    rng = np.random.default_rng(5)
    values = np.concatenate([table, mid, np.nextafter(mid, np.float32(2)), np.nextafter(mid, np.float32(-1)),
                             rng.random(4000, dtype=np.float32), np.float32([np.nan, -1, -0.0, 1.5, np.inf, -np.inf, 1e-30])])
    codes = meshstream.srgb_encode(values, table)
    nearest = np.abs(values[:-7, None].astype(np.float64) - table[None, :]).argmin(axis=1)  # argmin takes the first = lower
    assert np.array_equal(codes[:-7], nearest) and list(codes[-7:]) == [0, 0, 0, 255, 255, 0, 0]
    table.tofile(str(tmp_path / "table.bin"))
    values.astype(np.float32).tofile(str(tmp_path / "values.bin"))
    rc, _, err = native(harness, "srgb", tmp_path / "table.bin", tmp_path / "values.bin", tmp_path / "codes.bin")
    assert rc == 0, err[-300:]
    assert np.array_equal(np.fromfile(str(tmp_path / "codes.bin"), dtype=np.uint8), codes)
