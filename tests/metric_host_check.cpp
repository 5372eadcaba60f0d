// Stand-alone host program over csrc/metric_math.h, the header csrc/metrics.hip compiles (tests/test_metric_refs_cpu.py builds it
// with the host compiler and reads its output).
//   metric_host_check pairs LO HI     "P np round slot i j" for every even np in LO..HI, every round and slot
//   metric_host_check rot Z...        "R zeta t c s" for every zeta given (hexadecimal or decimal floats)
//   metric_host_check poly3 G D       "K value" of kid_poly3
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "metric_math.h"

int main(int argc, char** argv) {
  if (argc >= 4 && !std::strcmp(argv[1], "pairs")) {
    const int lo = std::atoi(argv[2]), hi = std::atoi(argv[3]);
    for (int np = lo; np <= hi; np += 2)
      for (int round = 0; round < np - 1; ++round)
        for (int slot = 0; slot < np / 2; ++slot) {
          int i, j;
          srgan::jacobi_pair(np, round, slot, &i, &j);
          std::printf("P %d %d %d %d %d\n", np, round, slot, i, j);
        }
    return 0;
  }
  if (argc >= 3 && !std::strcmp(argv[1], "rot")) {
    for (int k = 2; k < argc; ++k) {
      const float zeta = std::strtof(argv[k], nullptr);
      const srgan::JacobiRot r = srgan::jacobi_rotation_zeta(zeta);
      std::printf("R %a %a %a %a\n", (double)zeta, (double)r.t, (double)r.c, (double)r.s);
    }
    return 0;
  }
  if (argc == 4 && !std::strcmp(argv[1], "poly3")) {
    std::printf("K %a\n", (double)srgan::kid_poly3(std::strtof(argv[2], nullptr), std::atoi(argv[3])));
    return 0;
  }
  std::fprintf(stderr, "usage: metric_host_check pairs LO HI | rot ZETA... | poly3 G D\n");
  return 2;
}
