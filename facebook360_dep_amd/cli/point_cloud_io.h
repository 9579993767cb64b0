// Text side of ExportPointCloud / ImportPointCloud: the point formatter and the point-file reader. Host only.
#pragma once
#include <charconv>

#include "cli_common.h"

namespace cli {

// ---------------------------------------------------------------- writing (ExportPointCloud.cpp:139-178)
// fmt::format("{}", float): the shortest decimal that reads back as the same fp32 value, in fixed notation for
// 1e-4 <= |v| < 1e16 and in scientific notation with at least two exponent digits otherwise; no trailing ".0";
// nan / inf / -inf. (The reference does not pin its fmt version and older ones print "%g"-like text; see DESIGN.)
// Appends to `out`, returns the number of characters.
inline int format_float_shortest(float v, char* out) {
  if (v != v) {
    memcpy(out, "nan", 3);
    return 3;
  }
  char* p = out;
  if (std::signbit(v)) {
    *p++ = '-';
    v = -v;
  }
  if (std::isinf(v)) {
    memcpy(p, "inf", 3);
    return (int)(p + 3 - out);
  }
  if (v == 0) {
    *p++ = '0';
    return (int)(p - out);
  }
  char sci[32];  // d[.ddd]e[+-]XX: the shortest round-trip digits
  const std::to_chars_result r = std::to_chars(sci, sci + sizeof sci, v, std::chars_format::scientific);
  const char* e = sci;
  char digits[16];
  int nd = 0;
  for (; *e != 'e'; ++e) {
    if (*e != '.') {
      digits[nd++] = *e;
    }
  }
  int exp10 = 0;
  std::from_chars(e + (e[1] == '+' ? 2 : 1), r.ptr, exp10);
  if (exp10 < -4 || exp10 >= 16) {
    memcpy(p, sci, (size_t)(r.ptr - sci));
    return (int)(p + (r.ptr - sci) - out);
  }
  if (exp10 < 0) {
    *p++ = '0';
    *p++ = '.';
    for (int k = -1; k > exp10; --k) {
      *p++ = '0';
    }
    memcpy(p, digits, (size_t)nd);
    return (int)(p + nd - out);
  }
  for (int k = 0; k <= exp10; ++k) {
    *p++ = k < nd ? digits[k] : '0';
  }
  if (nd > exp10 + 1) {
    *p++ = '.';
    memcpy(p, digits + exp10 + 1, (size_t)(nd - exp10 - 1));
    p += nd - exp10 - 1;
  }
  return (int)(p - out);
}

// fmt::format("{:.0f}", 255 * c): the float product rounded to an integer, ties to even (the value is exact in binary,
// so this is what printf's "%.0f" prints too)
inline int format_color_255(float c, char* out) {
  const float v = 255 * c;
  if (!std::signbit(v) && v < 1e6f) {
    const unsigned u = (unsigned)nearbyintf(v);
    return (int)(std::to_chars(out, out + 16, u).ptr - out);
  }
  return snprintf(out, 48, "%.0f", (double)v);  // negative (-0 too), huge, nan / inf
}

constexpr int kPointLineMax = 3 * 20 + 3 * 48 + 16;
// "x y z 1 R G B\n" of one point (six floats: x y z r g b)
inline int format_point_line(const float* p, char* out) {
  char* q = out;
  for (int k = 0; k < 3; ++k) {
    q += format_float_shortest(p[k], q);
    *q++ = ' ';
  }
  *q++ = '1';
  for (int k = 3; k < 6; ++k) {
    *q++ = ' ';
    q += format_color_255(p[k], q);
  }
  *q++ = '\n';
  return (int)(q - out);
}

// ---------------------------------------------------------------- reading (PointCloudUtil.cpp:62-198)
// A .pcd file has PCL's 11-line header (verifyPCLHeader, extractPCLPointCount); anything else starts with one line that
// holds the point count (extractASCIIPointCount). Point k is read from line header + 1 + k, x y z as doubles, the rest
// of the line ignored. (The reference indexes its array by FILE LINE, :161-172, which leaves the first entries unset and
// writes past the end; that is not copied.) The file is streamed in blocks, so its size is not bounded by memory.
struct PointFileReader {
  std::string path;
  FILE* f = nullptr;
  long long count = 0, done = 0;
  std::string carry;  // text read but not parsed yet; starts at a line start
  bool eof = false;

  ~PointFileReader() {
    if (f) {
      fclose(f);
    }
  }
  bool read_line(std::string& line) {
    line.clear();
    int ch;
    bool any = false;
    while ((ch = fgetc(f)) != EOF) {
      any = true;
      if (ch == '\n') {
        break;
      }
      line.push_back((char)ch);
    }
    if (!line.empty() && line.back() == '\r') {
      line.pop_back();
    }
    return any;
  }
  static bool parse_count(const std::string& text, long long& out) {  // boost::lexical_cast<int>: the whole token
    const char* b = text.data();
    const char* e = b + text.size();
    if (b != e && *b == '+') {
      ++b;
    }
    int v = 0;
    const std::from_chars_result r = std::from_chars(b, e, v);
    if (r.ec != std::errc() || r.ptr != e || v < 0) {
      return false;
    }
    out = v;
    return true;
  }
  void open(const std::string& file) {
    path = file;
    f = fopen(file.c_str(), "rb");
    CHECK_MSG(f != nullptr, "File does not exist: " + file);
    std::string line;
    if (fs::path(file).extension() == ".pcd") {
      std::string fields, points, data;
      for (int n = 1; n <= 11; ++n) {
        CHECK_MSG(read_line(line), "PCL header: the file ends inside its 11-line header: " + file);
        (n == 3 ? fields : n == 10 ? points : n == 11 ? data : line) = line;
      }
      CHECK_MSG(fields.rfind("FIELDS x y z", 0) == 0, "PCL header: FIELDS must start with x y z");
      CHECK_MSG(data == "DATA ascii", "PCL header: DATA must be ascii");
      CHECK_MSG(points.rfind("POINTS", 0) == 0, "PCL header: expected point count in line 10, got " + points);
      CHECK_MSG(points.size() > 7 && points[6] == ' ' && parse_count(points.substr(7), count),
                "Could not parse point count from line " + points);
    } else {
      CHECK_MSG(read_line(line), "First line should contain point count: " + file);
      const size_t a = line.find_first_not_of(" \t"), b = line.find_last_not_of(" \t");
      CHECK_MSG(a != std::string::npos && parse_count(line.substr(a, b - a + 1), count),
                "First line should contain point count: " + line);
    }
  }
  static bool parse_xyz(const char* b, const char* e, double* xyz) {
    for (int k = 0; k < 3; ++k) {
      while (b < e && (*b == ' ' || *b == '\t')) {
        ++b;
      }
      if (b < e && *b == '+') {
        ++b;
      }
      const std::from_chars_result r = std::from_chars(b, e, xyz[k]);
      if (r.ec == std::errc::invalid_argument) {
        return false;
      }
      if (r.ec == std::errc::result_out_of_range) {  // strtod's answer: +-inf or a denormal / zero
        xyz[k] = strtod(std::string(b, r.ptr).c_str(), nullptr);
      }
      b = r.ptr;
    }
    return true;
  }
  // the next at most `maxPoints` points into xyz (rows of three doubles); returns how many (0 = all `count` are read).
  // Fewer lines in the file than the header's count is fatal.
  size_t next(IoPool& pool, size_t maxPoints, std::vector<double>& xyz) {
    const size_t want = (size_t)std::min<long long>((long long)maxPoints, count - done);
    if (want == 0) {
      return 0;
    }
    std::vector<size_t> starts;  // line starts inside `carry`, and one past the last line's newline
    starts.reserve(want + 1);
    size_t scanned = 0;
    starts.push_back(0);
    for (;;) {
      while (starts.size() <= want) {
        const void* nl = memchr(carry.data() + scanned, '\n', carry.size() - scanned);
        if (!nl) {
          scanned = carry.size();
          break;
        }
        scanned = (size_t)((const char*)nl - carry.data()) + 1;
        starts.push_back(scanned);
      }
      if (starts.size() > want) {
        break;
      }
      if (eof) {
        if (scanned == carry.size() && starts.back() < carry.size()) {  // a last line without a newline
          starts.push_back(carry.size());
          scanned = carry.size();
          if (starts.size() > want) {
            break;
          }
        }
        LOG_FATAL(fmt("Point count in header (%lld) does not match number of extracted points (%lld): %s", count,
                      done + (long long)starts.size() - 1, path.c_str()));
      }
      const size_t block = 8u << 20, old = carry.size();
      carry.resize(old + block);
      const size_t got = fread(&carry[old], 1, block, f);
      carry.resize(old + got);
      eof = got < block;
    }
    xyz.resize(want * 3);
    std::atomic<long long> bad{-1};
    parallel_rows(pool, (int)want, [&](int a, int b) {
      for (int k = a; k < b; ++k) {
        if (!parse_xyz(carry.data() + starts[k], carry.data() + starts[k + 1], &xyz[(size_t)k * 3])) {
          bad = k;
        }
      }
    });
    if (bad >= 0) {
      LOG_FATAL(fmt("cannot read x y z of point %lld: %s", done + bad, path.c_str()));
    }
    carry.erase(0, starts[want]);
    done += (long long)want;
    return want;
  }
};

}  // namespace cli
