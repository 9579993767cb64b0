// Reading the fused mesh stream back: the catalog fused.json (VideoFile::parseCatalog, source/render/VideoFile.h:140-165)
// and the striped files fused_<i>.bin (StripedFile::calcStripe, source/mesh_stream/StripedFile.h) that ConvertToBinary's
// fusion writes; or the unfused <bin>/<camera>/<frame>.<ext> tree. Every offset and size of the catalog is held against
// the strip files' real lengths before a byte is copied. The sRGB code of a linear value (the inverse of the decode table
// the renderer uses). Definitions: DESIGN §8.11.
#pragma once
#include "cli_common.h"

namespace cli {

constexpr uint64_t kMeshStripe = 512 * 1024;  // StripedFile's stripe

struct MeshStreamEntry {
  uint64_t offset = 0, size = 0;
  bool present = false;
};
// one camera of one frame: the byte ranges of its files in the striped stream, by extension
struct MeshStreamCamera {
  std::map<std::string, MeshStreamEntry> files;  // ".vtx", ".idx", ".rgba", ".bc7"
};
struct MeshCatalog {
  std::map<std::string, std::map<std::string, MeshStreamCamera>> frames;  // frame name -> camera id
};

// a non-negative whole number that a double holds exactly
inline uint64_t catalog_integer(const Json* j, const std::string& what) {
  CHECK_MSG(j && j->kind == Json::Num && j->num >= 0 && j->num <= 9007199254740992.0 && j->num == std::floor(j->num),
            "Malformed catalog file: " + what + " is not a whole number");
  return (uint64_t)j->num;
}

inline MeshCatalog parse_mesh_catalog(const std::string& text, const std::string& name) {
  CHECK_MSG(!text.empty(), "could not read catalog file: " + name);
  JsonParser jp(text);
  Json root = jp.value();
  CHECK_MSG(root.kind == Json::Obj, "Malformed catalog file: " + name);
  const Json* frames = root.find("frames");
  if (!root.find("metadata")) {  // the legacy form: the frames themselves, native endianness assumed
    LOG_WARNING("No metadata found");
    CHECK_MSG(!frames, "Malformed catalog file: " + name);
    frames = &root;
  } else {
    const Json* little = root.at("metadata").find("isLittleEndian");
    CHECK_MSG(little && little->kind == Json::Bool, "Malformed catalog file: metadata.isLittleEndian");
    const uint16_t probe = 1;
    const bool native = *reinterpret_cast<const unsigned char*>(&probe) == 1;
    CHECK_MSG(little->boolean == native, "Endianness mismatch between video file and native platform");
    CHECK_MSG(frames, "Malformed catalog file: no frames in " + name);
  }
  CHECK_MSG(frames->kind == Json::Obj, "Malformed catalog file: frames");
  MeshCatalog out;
  for (const auto& frame : frames->obj) {
    CHECK_MSG(frame.second.kind == Json::Obj, "Malformed catalog file: frame " + frame.first);
    auto& cams = out.frames[frame.first];
    for (const auto& cam : frame.second.obj) {
      CHECK_MSG(cam.second.kind == Json::Obj, "Malformed catalog file: camera " + cam.first);
      MeshStreamCamera& c = cams[cam.first];
      for (const auto& file : cam.second.obj) {
        if (file.second.kind != Json::Obj) {
          continue;  // the camera's own "offset" and "size"
        }
        MeshStreamEntry e;
        e.offset = catalog_integer(file.second.find("offset"), frame.first + "/" + cam.first + "/" + file.first + " offset");
        e.size = catalog_integer(file.second.find("size"), frame.first + "/" + cam.first + "/" + file.first + " size");
        e.present = true;
        c.files[file.first] = e;
      }
    }
  }
  return out;
}
inline MeshCatalog load_mesh_catalog(const fs::path& path) {
  return parse_mesh_catalog(read_file_or_empty(path), path.string());
}

// The strip files of one stream. read() is the inverse of the writer's addFile: global stripe s lies in disk s % N at
// local stripe s / N.
struct StripedReader {
  std::vector<std::string> names;
  std::vector<uint64_t> lengths;
  explicit StripedReader(const std::vector<std::string>& files) : names(files) {
    CHECK_MSG(!files.empty(), "no strip files");
    for (const std::string& f : files) {
      std::error_code ec;
      const uintmax_t n = fs::file_size(f, ec);
      CHECK_MSG(!ec, "cannot open strip file " + f);
      lengths.push_back((uint64_t)n);
    }
  }
  // every byte of [offset, offset + size) lies inside its strip file; fatal, by name, otherwise
  void check(uint64_t offset, uint64_t size, const std::string& what) const {
    CHECK_MSG(size <= UINT64_MAX - offset, what + ": offset + size overflows");
    const uint64_t n = names.size();
    for (uint64_t at = offset, left = size; left > 0;) {
      const uint64_t stripe = at / kMeshStripe, within = at % kMeshStripe, take = std::min(left, kMeshStripe - within);
      const uint64_t local = (stripe / n) * kMeshStripe + within;
      const uint64_t have = lengths[stripe % n];
      CHECK_MSG(local <= have && take <= have - local,
                fmt("%s: bytes %llu..%llu lie past the end of %s (%llu bytes)", what.c_str(), (unsigned long long)at,
                    (unsigned long long)(at + take), names[stripe % n].c_str(), (unsigned long long)have));
      at += take;  // (the walk ends at the first stripe past a file's end, so the files' lengths bound it)
      left -= take;
    }
  }
  std::vector<uint8_t> read(uint64_t offset, uint64_t size, const std::string& what) const {
    check(offset, size, what);
    std::vector<uint8_t> out((size_t)size);
    std::vector<FILE*> disks(names.size(), nullptr);
    bool ok = true;
    const uint64_t n = names.size();
    for (uint64_t at = offset, done = 0; ok && done < size;) {
      const uint64_t stripe = at / kMeshStripe, within = at % kMeshStripe, take = std::min(size - done, kMeshStripe - within);
      FILE*& disk = disks[stripe % n];
      if (!disk) {
        disk = fopen(names[stripe % n].c_str(), "rb");
      }
      ok = disk && fseeko(disk, (off_t)((stripe / n) * kMeshStripe + within), SEEK_SET) == 0 &&
           fread(out.data() + done, 1, (size_t)take, disk) == take;
      at += take;
      done += take;
    }
    for (FILE* d : disks) {
      if (d) {
        fclose(d);
      }
    }
    CHECK_MSG(ok, what + ": failed to read the strip files");
    return out;
  }
};

// one camera's files of one frame, as bytes
struct MeshStreamFrameCamera {
  std::vector<uint8_t> vtx, idx, rgba;
};

// the files the renderer needs of (frame, camera), refused by name when the catalog does not hold them
inline const MeshStreamCamera& catalog_camera(const MeshCatalog& catalog, const std::string& frame, const std::string& cam) {
  const auto f = catalog.frames.find(frame);
  CHECK_MSG(f != catalog.frames.end(), "frame " + frame + " is not in the catalog");
  const auto c = f->second.find(cam);
  CHECK_MSG(c != f->second.end(), "camera " + cam + " of the rig is missing from frame " + frame + " of the catalog");
  const MeshStreamCamera& entry = c->second;
  if (!entry.files.count(".rgba")) {
    CHECK_MSG(!entry.files.count(".bc7"), "frame " + frame + " holds " + cam + ".bc7 but no .rgba: bc7 colour is not built; write "
                                          "the stream with --output_formats=idx,vtx,rgba");
  }
  for (const char* ext : {".vtx", ".idx", ".rgba"}) {
    CHECK_MSG(entry.files.count(ext), "frame " + frame + ", camera " + cam + ": the catalog holds no " + ext);
  }
  return entry;
}

// sizes a mesh's files must have: whole vertices, whole triangles, w x h RGBA bytes
inline void check_mesh_sizes(uint64_t vtx, uint64_t idx, uint64_t rgba, int w, int h, const std::string& what) {
  CHECK_MSG(vtx % 12 == 0, what + ": the .vtx size is not a multiple of 12 bytes");
  CHECK_MSG(idx % 12 == 0, what + ": the .idx size is not a multiple of 12 bytes (three uint32 per triangle)");
  CHECK_MSG(rgba == (uint64_t)w * h * 4,
            fmt("%s: the .rgba holds %llu bytes, the camera's %dx%d colour needs %llu", what.c_str(), (unsigned long long)rgba, w, h,
                (unsigned long long)((uint64_t)w * h * 4)));
}

// ---- sRGB: the code of a linear value = the code whose decoded value is nearest, the lower code on a tie. The decoded
// values increase with the code, so the code is found by bisection on the 255 midpoints; no pow per pixel.
struct SrgbEncoder {
  float value[256];
  explicit SrgbEncoder(const float* table) { memcpy(value, table, sizeof value); }
  uint8_t operator()(float v) const {
    if (!(v > value[0])) {  // NaN, negative, zero
      return 0;
    }
    int lo = 0, hi = 255;  // value[lo] < v; the answer is in [lo, hi]
    while (hi - lo > 1) {
      const int mid = (lo + hi) / 2;
      if (value[mid] < v) {
        lo = mid;
      } else {
        hi = mid;
      }
    }
    // value[lo] < v <= value[hi] (or v beyond the last code): the nearer one, the lower on a tie; distances in double
    return (double)v - value[lo] <= (double)value[hi] - v ? (uint8_t)lo : (uint8_t)hi;
  }
};

}  // namespace cli
