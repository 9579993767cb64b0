"""Reader of the fused mesh stream ConvertToBinary writes: the catalog fused.json (VideoFile::parseCatalog,
source/render/VideoFile.h:140-165) and the striped files fused_<i>.bin (StripedFile::calcStripe), or the unfused
<bin>/<camera>/<frame>.<ext> tree; and the sRGB code of a linear value as MeshStreamRenderer's png output encodes it.
The same rules as cli/mesh_stream_io.h: every offset and size is held against the strip files' real lengths before a
byte is read."""
import json
import os
import sys

import numpy as np

STRIPE = 512 * 1024


class MeshStreamError(ValueError):
    pass


def parse_catalog(text):
    """-> {frame: {camera: {extension: (offset, size)}}}; the legacy form without `metadata` is the frames themselves"""
    try:
        root = json.loads(text)
    except (ValueError, RecursionError) as e:  # (a file of a hundred thousand brackets)
        raise MeshStreamError("Malformed catalog file: %s" % e)
    if not isinstance(root, dict):
        raise MeshStreamError("Malformed catalog file")
    if "metadata" not in root:
        if "frames" in root:
            raise MeshStreamError("Malformed catalog file")
        frames = root  # native endianness assumed
    else:
        little = root["metadata"].get("isLittleEndian") if isinstance(root["metadata"], dict) else None
        if not isinstance(little, bool):
            raise MeshStreamError("Malformed catalog file: metadata.isLittleEndian")
        if little != (sys.byteorder == "little"):
            raise MeshStreamError("Endianness mismatch between video file and native platform")
        frames = root.get("frames")
    if not isinstance(frames, dict):
        raise MeshStreamError("Malformed catalog file: frames")
    out = {}
    for frame, cams in frames.items():
        if not isinstance(cams, dict):
            raise MeshStreamError("Malformed catalog file: frame %s" % frame)
        out[frame] = {}
        for cam, files in cams.items():
            if not isinstance(files, dict):
                raise MeshStreamError("Malformed catalog file: camera %s" % cam)
            entry = out[frame][cam] = {}
            for ext, where in files.items():
                if not isinstance(where, dict):
                    continue  # the camera's own "offset" and "size"
                pair = (where.get("offset"), where.get("size"))
                if not all(isinstance(v, int) and not isinstance(v, bool) and v >= 0 for v in pair):
                    raise MeshStreamError("Malformed catalog file: %s/%s/%s is not a pair of whole numbers" % (frame, cam, ext))
                entry[ext] = pair
    return out


class StripedReader:
    """read(offset, size) over N strip files: global stripe s lies in file s % N at local stripe s // N"""

    def __init__(self, strip_files):
        self.names = list(strip_files)
        if not self.names:
            raise MeshStreamError("no strip files")
        for name in self.names:
            if not os.path.isfile(name):
                raise MeshStreamError("cannot open strip file %s" % name)
        self.lengths = [os.path.getsize(name) for name in self.names]

    def _pieces(self, offset, size, what):
        n = len(self.names)
        at, left = offset, size
        while left > 0:
            stripe, within = divmod(at, STRIPE)
            take = min(left, STRIPE - within)
            local = (stripe // n) * STRIPE + within
            if local + take > self.lengths[stripe % n]:
                raise MeshStreamError("%s: bytes %d..%d lie past the end of %s (%d bytes)"
                                      % (what, at, at + take, self.names[stripe % n], self.lengths[stripe % n]))
            yield stripe % n, local, take
            at += take
            left -= take

    def read(self, offset, size, what="read"):
        pieces = list(self._pieces(offset, size, what))  # all of it is checked before a byte is read
        out = bytearray()
        for disk, local, take in pieces:
            with open(self.names[disk], "rb") as f:
                f.seek(local)
                out += f.read(take)
        if len(out) != size:
            raise MeshStreamError("%s: failed to read the strip files" % what)
        return bytes(out)


def _arrays(vtx, idx, rgba, resolution, what):
    w, h = resolution
    if len(vtx) % 12:
        raise MeshStreamError("%s: the .vtx size is not a multiple of 12 bytes" % what)
    if len(idx) % 12:
        raise MeshStreamError("%s: the .idx size is not a multiple of 12 bytes (three uint32 per triangle)" % what)
    if len(rgba) != w * h * 4:
        raise MeshStreamError("%s: the .rgba holds %d bytes, the camera's %dx%d colour needs %d" % (what, len(rgba), w, h, w * h * 4))
    return (np.frombuffer(vtx, dtype="<f4").reshape(-1, 3), np.frombuffer(idx, dtype="<u4"),
            np.frombuffer(rgba, dtype=np.uint8).reshape(h, w, 4))


class MeshStream:
    """A fused stream: MeshStream(catalog path, strip files).mesh(frame, camera id, (w, h)) -> (vtx, idx, rgba)"""

    def __init__(self, catalog, strip_files):
        with open(catalog) as f:
            self.catalog = parse_catalog(f.read())
        self.reader = StripedReader(strip_files)

    def read(self, frame, cam, ext):
        if frame not in self.catalog:
            raise MeshStreamError("frame %s is not in the catalog" % frame)
        if cam not in self.catalog[frame]:
            raise MeshStreamError("camera %s of the rig is missing from frame %s of the catalog" % (cam, frame))
        files = self.catalog[frame][cam]
        if ext not in files:
            if ext == ".rgba" and ".bc7" in files:
                raise MeshStreamError("frame %s holds %s.bc7 but no .rgba: bc7 colour is not built; write the stream with "
                                      "--output_formats=idx,vtx,rgba" % (frame, cam))
            raise MeshStreamError("frame %s, camera %s: the catalog holds no %s" % (frame, cam, ext))
        return self.reader.read(*files[ext], what="%s/%s%s" % (frame, cam, ext))

    def mesh(self, frame, cam, resolution):
        return _arrays(*(self.read(frame, cam, ext) for ext in (".vtx", ".idx", ".rgba")), resolution, "%s/%s" % (frame, cam))


def bin_mesh(bin_dir, frame, cam, resolution):
    """the same arrays from an unfused <bin>/<camera>/<frame>.<ext> tree"""
    blobs = []
    for ext in (".vtx", ".idx", ".rgba"):
        path = os.path.join(bin_dir, cam, frame + ext)
        if not os.path.isfile(path):
            raise MeshStreamError("Missing file: %s" % path)
        with open(path, "rb") as f:
            blobs.append(f.read())
    return _arrays(*blobs, resolution, "%s/%s" % (frame, cam))


def srgb_encode(linear, table):
    """the 8-bit sRGB code of linear values: the code whose decoded value (table[code]) is nearest, the lower code on a
    tie; NaN and values <= 0 give 0"""
    table = np.asarray(table, dtype=np.float32)
    v = np.asarray(linear, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        hi = np.clip(np.searchsorted(table, np.where(np.isnan(v), 0, v), side="left"), 1, 255)  # table[hi - 1] < v <= table[hi]
        lo = hi - 1
        d_lo, d_hi = v.astype(np.float64) - table[lo], table[hi].astype(np.float64) - v
        code = np.where(d_lo <= d_hi, lo, hi)
        return np.where(v > table[0], code, 0).astype(np.uint8)
