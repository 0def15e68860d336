// Stand-alone host driver of csrc/kernels/pack58.h for tests/test_pack58_cpu.py (built there with
// -fsanitize=address,undefined).  in: int32 {ld, e0, nrows} then nrows * ld doubles.  out, per row: the 7424-byte
// packed block, one byte "every value decodes to itself", and the ld doubles decoded from the block.
#include <cstdio>
#include <cstring>
#include <vector>

#include "kernels/pack58.h"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = std::fopen(argv[1], "rb");
  FILE* out = std::fopen(argv[2], "wb");
  if (!in || !out) return 3;
  int hdr[3];
  if (std::fread(hdr, sizeof(int), 3, in) != 3) return 4;
  const int ld = hdr[0], e0 = hdr[1], nrows = hdr[2];
  if (ld < 1 || ld > eh::p58::kCols || nrows < 0) return 5;
  std::vector<uint64_t> x(ld), back(ld);
  std::vector<uint32_t> row(eh::p58::kRowBytes / 4);
  for (int r = 0; r < nrows; ++r) {
    if (std::fread(x.data(), 8, ld, in) != static_cast<size_t>(ld)) return 6;
    std::memset(row.data(), 0xAB, eh::p58::kRowBytes);  // every byte of the block must be written
    const unsigned char exact = eh::p58::pack_row(x.data(), ld, e0, row.data()) ? 1 : 0;
    eh::p58::unpack_row(row.data(), ld, e0, back.data());
    std::fwrite(row.data(), 1, eh::p58::kRowBytes, out);
    std::fwrite(&exact, 1, 1, out);
    std::fwrite(back.data(), 8, ld, out);
  }
  std::fclose(in);
  return std::fclose(out) == 0 ? 0 : 7;
}
