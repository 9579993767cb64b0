// JSON output and the rig writer (Camera::saveRig), shared by the executables that write a rig file: ConvertToBinary's
// fused rig and RigSimulator's --rig_out.
#pragma once
#include "cli_common.h"

namespace cli {

// ---------------------------------------------------------------- JSON out (folly::json::serialize, sorted + pretty)
// folly is not available to pin its pretty-printer's white space against: the form here is sorted keys, two-space
// indentation, one element per line, "key": value, doubles with a fixed number of digits after the point.
struct JsonOut {
  enum Kind { Int, Dbl, Bool, Str, Arr, Obj } kind = Int;
  uint64_t i = 0;
  double d = 0;
  bool b = false;
  std::string s;
  std::vector<JsonOut> arr;
  std::map<std::string, JsonOut> obj;  // (sorted)
  static JsonOut integer(uint64_t v) { JsonOut j; j.kind = Int; j.i = v; return j; }
  static JsonOut number(double v) { JsonOut j; j.kind = Dbl; j.d = v; return j; }
  static JsonOut boolean(bool v) { JsonOut j; j.kind = Bool; j.b = v; return j; }
  static JsonOut string(const std::string& v) { JsonOut j; j.kind = Str; j.s = v; return j; }
  static JsonOut array() { JsonOut j; j.kind = Arr; return j; }
  static JsonOut object() { JsonOut j; j.kind = Obj; return j; }
  static JsonOut vector(const double* v, int n) {
    JsonOut j = array();
    for (int k = 0; k < n; ++k) {
      j.arr.push_back(number(v[k]));
    }
    return j;
  }
  static void quote(const std::string& v, std::string& out) {
    out += '"';
    for (char ch : v) {
      if (ch == '"' || ch == '\\') {
        out += '\\';
      }
      out += ch;
    }
    out += '"';
  }
  // digits <= 0 (saveRig's default, folly's shortest form): the fewest significant digits that read back as the same
  // double, with ".0" after a whole number so that it stays a double for every reader
  static std::string shortest(double v) {
    std::string s;
    for (int p = 1; p <= 17; ++p) {
      s = fmt("%.*g", p, v);
      if (std::strtod(s.c_str(), nullptr) == v) {
        break;
      }
    }
    return s.find_first_of(".eni") == std::string::npos ? s + ".0" : s;
  }
  void write(std::string& out, int digits, int indent = 0) const {
    const std::string pad((size_t)indent + 2, ' '), close((size_t)indent, ' ');
    switch (kind) {
      case Int: out += std::to_string(i); break;
      case Dbl: out += digits > 0 ? fmt("%.*f", digits, d) : shortest(d); break;
      case Bool: out += b ? "true" : "false"; break;
      case Str: quote(s, out); break;
      case Arr:
        if (arr.empty()) {
          out += "[]";
          break;
        }
        out += "[\n";
        for (size_t k = 0; k < arr.size(); ++k) {
          out += pad;
          arr[k].write(out, digits, indent + 2);
          out += k + 1 < arr.size() ? ",\n" : "\n";
        }
        out += close + "]";
        break;
      case Obj: {
        if (obj.empty()) {
          out += "{}";
          break;
        }
        out += "{\n";
        size_t k = 0;
        for (const auto& kv : obj) {
          out += pad;
          quote(kv.first, out);
          out += ": ";
          kv.second.write(out, digits, indent + 2);
          out += ++k < obj.size() ? ",\n" : "\n";
        }
        out += close + "}";
        break;
      }
    }
  }
};

static void write_text(const fs::path& path, const std::string& text) {
  std::ofstream f(path, std::ios::binary);
  f.write(text.data(), (std::streamsize)text.size());
  f.close();
  CHECK_MSG(f.good(), "failed to write: " + path.string());
}

// Camera::serialize (Camera.cpp:158-177) + Camera::saveRig (:293-313). The rotation rows are written as the rig file
// held them (the reference re-unitarises them through Eigen::AngleAxis first: a change far below the ten digits
// written for a rig that passes its isUnitary check). The optional "group" is not part of the C-ABI's camera: it is
// read from the rig file a second time (rig_groups) and handed in by camera id.
static void save_rig(const fs::path& path, const std::vector<derp_camera_desc>& rig,
                     const std::map<std::string, std::string>& groups, int digits,
                     const std::vector<std::string>& comments = {}) {
  static const char* kTypes[] = {"FTHETA", "RECTILINEAR", "EQUISOLID", "ORTHOGRAPHIC"};
  JsonOut root = JsonOut::object();
  JsonOut cams = JsonOut::array();
  for (const derp_camera_desc& c : rig) {
    JsonOut j = JsonOut::object();
    j.obj["version"] = JsonOut::integer(1);
    const int type = c.type == DERP_FTHETA ? 0 : c.type == DERP_RECTILINEAR ? 1 : c.type == DERP_EQUISOLID ? 2 : 3;
    j.obj["type"] = JsonOut::string(kTypes[type]);
    j.obj["origin"] = JsonOut::vector(c.origin, 3);
    j.obj["forward"] = JsonOut::vector(c.forward, 3);
    j.obj["up"] = JsonOut::vector(c.up, 3);
    j.obj["right"] = JsonOut::vector(c.right, 3);
    j.obj["resolution"] = JsonOut::vector(c.resolution, 2);
    j.obj["focal"] = JsonOut::vector(c.focal, 2);
    j.obj["id"] = JsonOut::string(c.id);
    if (c.has_principal && (c.principal[0] != c.resolution[0] / 2 || c.principal[1] != c.resolution[1] / 2)) {
      j.obj["principal"] = JsonOut::vector(c.principal, 2);
    }
    if (c.has_distortion && (c.distortion[0] != 0 || c.distortion[1] != 0 || c.distortion[2] != 0)) {
      j.obj["distortion"] = JsonOut::vector(c.distortion, 3);
    }
    if (c.has_fov) {  // setFov keeps cos(fov); isDefaultFov compares it with the type's default; getFov = acos of it
      const double cosFov = std::cos(c.fov);
      const double dflt = (type == 1 || type == 3) ? 0 : -1;
      if (cosFov != dflt) {
        j.obj["fov"] = JsonOut::number(std::acos(cosFov));
      }
    }
    const auto group = groups.find(c.id);
    if (group != groups.end() && !group->second.empty()) {
      j.obj["group"] = JsonOut::string(group->second);
    }
    cams.arr.push_back(j);
  }
  root.obj["cameras"] = cams;
  if (!comments.empty()) {
    JsonOut list = JsonOut::array();
    for (const std::string& line : comments) {
      list.arr.push_back(JsonOut::string(line));
    }
    root.obj["comments"] = list;
  }
  std::string text;
  root.write(text, digits);
  write_text(path, text + "\n");
}

}  // namespace cli
