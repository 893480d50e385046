// TEST INFRASTRUCTURE: pion_host_read_cooling_curve and the curve functions of pion_amd/host/cooling_tables.cpp with a
// main of their own, so that they can run under the address and undefined-behaviour sanitisers as a plain executable
// (tests/test_cooling_forms.py compiles this file together with cooling_tables.cpp; nothing is preloaded).
//   cooling_curve_probe FILE...   one line per file: "ok <n> <Lambda(1e5 K)>" or "bad <message>"; exit status 0
#include <cstdio>
#include <vector>

#include "../../include/pion_host.h"

int main(int argc, char **argv)
{
  for (int i = 1; i < argc; i++) {
    // (arrays of exactly max_n: a write past the count the reader was given is an error the sanitiser sees)
    for (int max_n : {256, 5}) {
      std::vector<double> x(max_n), y(max_n), c(max_n);
      int n = -1;
      char err[64];   // (shorter than most messages: the reader must truncate)
      if (pion_host_read_cooling_curve(argv[i], max_n, x.data(), y.data(), &n, err, (int)sizeof err) != 0) {
        std::printf("bad %s\n", err);
        continue;
      }
      if (pion_host_build_cooling_curve(n, x.data(), y.data(), c.data()) != 0
          || pion_host_cooling_curve_set(n, x.data(), y.data(), 8.0, (y[n - 1] - y[n - 2]) / (x[n - 1] - x[n - 2])) != 0) {
        std::printf("bad curve the reader accepted was refused\n");
        return 1;
      }
      std::printf("ok %d %.17g\n", n, pion_host_cooling_curve_rate(1.0e5));
    }
  }
  return 0;
}
