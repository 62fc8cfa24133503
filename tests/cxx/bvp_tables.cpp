// Prints the host tables of the batched boundary value problem solver (uammd_amd/csrc/bvp_host.hpp) for the systems on the command
// line:  bvp_tables nz H  k tfi tsi bfi bsi  [k tfi tsi bfi bsi ...]
// One line per table row: name, row index, then one value per system.  Plain C++: tests/test_chebyshev_bvp_cpu.py builds it with the
// address and undefined-behaviour sanitizers and compares the output with the NumPy restatement.  Exit status 2 with the message on
// stderr when the batch is refused.
#include "../../uammd_amd/csrc/bvp_host.hpp"

#include <cstdlib>

int main(int argc, char **argv) {
  if (argc < 8 || (argc - 3) % 5 != 0) {
    std::fprintf(stderr, "usage: %s nz H  k tfi tsi bfi bsi ...\n", argv[0]);
    return 1;
  }
  const int nz = std::atoi(argv[1]);
  const double H = std::atof(argv[2]);
  const int nsys = (argc - 3) / 5;
  std::vector<double> par[5];
  for (int s = 0; s < nsys; ++s)
    for (int p = 0; p < 5; ++p) par[p].push_back(std::atof(argv[3 + 5 * s + p]));
  uammd_hip::bvp::HostTables t;
  std::string err;
  if (uammd_hip::bvp::precompute(nsys, nz, H, par[0].data(), par[1].data(), par[2].data(), par[3].data(), par[4].data(), t, err)) {
    std::fprintf(stderr, "%s\n", err.c_str());
    return 2;
  }
  const struct { const char *name; const std::vector<double> *v; } all[] = {{"beta", &t.beta}, {"diagonal_p2", &t.diagonal_p2},
      {"diagonal_m2", &t.diagonal_m2}, {"cinvA", &t.cinvA}, {"m22", &t.m22}, {"kH2", &t.kH2}};
  for (const auto &e : all) {
    const size_t rows = e.v->size() / nsys;
    for (size_t i = 0; i < rows; ++i) {
      std::printf("%s %zu", e.name, i);
      for (int s = 0; s < nsys; ++s) std::printf(" %.17g", (*e.v)[s + (size_t)nsys * i]);
      std::printf("\n");
    }
  }
  return 0;
}
