// Writes the host tables of csrc/dft_tables.h to a file, for tests/test_dft_tables_host.py:
//   dft_tables_dump N WIN OFFSET T4_SCALE OUT
// OUT holds nine uint64 -- the offsets (in floats) of win, wsq, twc, tws, T1, T2, T3, T4 and the float count -- then the floats.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../../tensorflowasr_amd/csrc/dft_tables.h"

int main(int argc, char** argv) {
  if (argc != 6) {
    std::fprintf(stderr, "usage: %s N WIN OFFSET T4_SCALE OUT\n", argv[0]);
    return 2;
  }
  const int N = std::atoi(argv[1]), win = std::atoi(argv[2]), offset = std::atoi(argv[3]);
  const double t4_scale = std::strtod(argv[4], nullptr);
  if ((N != 512 && N != 1024 && N != 2048) || win < 1 || offset < 0 || offset + win > N) {
    std::fprintf(stderr, "need N in {512, 1024, 2048} and 0 <= OFFSET, 1 <= WIN, OFFSET + WIN <= N\n");
    return 2;
  }
  std::vector<float> buf;
  uint64_t head[9];
  head[0] = buf.size();
  mi355::append_hann(win, N, offset, false, &buf);
  head[1] = buf.size();
  mi355::append_hann(win, N, offset, true, &buf);
  const mi355::DftOffsets at = mi355::append_dft_tables(N, t4_scale, &buf);
  head[2] = at.twc; head[3] = at.tws; head[4] = at.T1; head[5] = at.T2; head[6] = at.T3; head[7] = at.T4;
  head[8] = buf.size();
  std::FILE* f = std::fopen(argv[5], "wb");
  if (!f) {
    std::perror(argv[5]);
    return 1;
  }
  const bool ok = std::fwrite(head, sizeof(head), 1, f) == 1 && std::fwrite(buf.data(), sizeof(float), buf.size(), f) == buf.size();
  return std::fclose(f) == 0 && ok ? 0 : 1;
}
