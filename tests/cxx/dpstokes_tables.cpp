// Prints the host tables of the doubly periodic Stokes solver's wall correction (uammd_amd/csrc/dpstokes_host.hpp): the inverses of the
// slit matrices and the rows of the k = 0 solve.  Plain C++, no device: tests/test_dpstokes_cpu.py builds it with the address and
// undefined-behaviour sanitizers and compares what it prints with numpy.
//   dpstokes_tables nx ny Lx Ly viscosity H nz
// prints   inv <s> <128 numbers: re, im of the 64 entries, row major>     for every wave number s != 0
//          zero <mode> <2 nz numbers: the two rows C> <4 numbers: the 2 x 2 matrix -D>   for mode 1 (bottom) and 2 (slit)
//          singular <message>     what a singular matrix is refused with (a 2 x 2 one, inverted as the 8 x 8 ones are)
#include "../../uammd_amd/csrc/dpstokes_host.hpp"

#include <cstdlib>

int main(int argc, char **argv) {
  using namespace uammd_hip;
  if (argc != 8) { std::fprintf(stderr, "usage: %s nx ny Lx Ly viscosity H nz\n", argv[0]); return 2; }
  const int nx = std::atoi(argv[1]), ny = std::atoi(argv[2]), nz = std::atoi(argv[7]);
  const double Lx = std::atof(argv[3]), Ly = std::atof(argv[4]), mu = std::atof(argv[5]), H = std::atof(argv[6]);
  std::vector<dps::cplx> inv;
  std::string err;
  if (dps::slit_inverses(nx, ny, Lx, Ly, mu, H, inv, err)) { std::fprintf(stderr, "%s\n", err.c_str()); return 1; }
  for (int s = 1; s < nx * ny; ++s) {
    std::printf("inv %d", s);
    for (int n = 0; n < 64; ++n) std::printf(" %.17g %.17g", inv[(size_t)64 * s + n].real(), inv[(size_t)64 * s + n].imag());
    std::printf("\n");
  }
  for (int mode = dps::kBottom; mode <= dps::kSlit; ++mode) {
    bvp::HostTables t;
    if (dps::zero_mode_rows(mode, nz, 0.5 * H, t, err)) { std::fprintf(stderr, "%s\n", err.c_str()); return 1; }
    std::printf("zero %d", mode);
    for (int i = 0; i < 2 * nz; ++i) std::printf(" %.17g", t.cinvA[i]);
    for (int i = 0; i < 4; ++i) std::printf(" %.17g", t.m22[i]);
    std::printf("\n");
  }
  dps::cplx S[4] = {1.0, 2.0, 2.0, 4.0}, Sinv[4];
  std::printf("singular %s\n", dps::invert(2, S, Sinv) ? "inverted" : "refused");
  return 0;
}
