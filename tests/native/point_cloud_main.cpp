// Test harness (CPU only) for cli/point_cloud_io.h. usage:
//   point_cloud_main read <file> <chunk>   -> "ok <count>" and one "%.17g %.17g %.17g" line per point, read in chunks
//   point_cloud_main float                 -> one formatted line per hexadecimal fp32 bit pattern on stdin
//   point_cloud_main color                 -> one "%.0f"-style line of 255 * c per hexadecimal fp32 bit pattern on stdin
// A file the reader refuses ends the process the way the executables end: "F... Check failed" / a fatal line, exit 1.
#include <cstdio>

#include "../../facebook360_dep_amd/cli/point_cloud_io.h"

int main(int argc, char** argv) {
  if (argc < 2) {
    return 2;
  }
  const std::string kind = argv[1];
  if (kind == "read" && argc >= 4) {
    cli::IoPool pool(2);
    cli::PointFileReader reader;
    reader.open(argv[2]);
    printf("ok %lld\n", reader.count);
    std::vector<double> xyz;
    while (const size_t n = reader.next(pool, (size_t)atoi(argv[3]), xyz)) {
      for (size_t k = 0; k < n; ++k) {
        printf("%.17g %.17g %.17g\n", xyz[3 * k], xyz[3 * k + 1], xyz[3 * k + 2]);
      }
    }
    return 0;
  }
  unsigned bits;
  char buf[64];
  while (scanf("%x", &bits) == 1) {
    float v;
    memcpy(&v, &bits, 4);
    const int n = kind == "float" ? cli::format_float_shortest(v, buf) : cli::format_color_255(v, buf);
    printf("%.*s\n", n, buf);
  }
  return 0;
}
