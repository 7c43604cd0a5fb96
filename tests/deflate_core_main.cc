// Host driver of csrc/deflate_core.h for tests/test_deflate_core_cpu.py and tests/test_gpu_deflate.py:
//   deflate_core_main <in_dir> <out_dir>
// compresses every file of in_dir (raw data, at most 0xff00 bytes) into one BGZF member and writes it under the
// same name into out_dir.  The input and the member live in heap blocks of their exact sizes (n and n + 31, the
// bound the core states), so AddressSanitizer sees any access one byte outside them.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <filesystem>
#include <fstream>
#include <string>
#include <vector>

#include "deflate_core.h"

using namespace snvrag;

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::vector<std::string> names;
  for (const auto& e : std::filesystem::directory_iterator(argv[1])) names.push_back(e.path().filename().string());
  std::sort(names.begin(), names.end());
  DeflState* state = new DeflState;
  for (const std::string& name : names) {
    std::ifstream f(std::filesystem::path(argv[1]) / name, std::ios::binary);
    std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    if (raw.size() > (size_t)DEFL_MAX_IN) return 3;
    const int n = (int)raw.size();
    uint8_t* in = new uint8_t[n];
    if (n) std::memcpy(in, raw.data(), raw.size());
    uint8_t* out = new uint8_t[n + 5 + DEFL_FRAME];
    DeflSerial one;
    const int len = defl_member(one, *state, in, n, out);
    if (len < DEFL_FRAME + 2 || len > n + 5 + DEFL_FRAME) return 4;
    std::ofstream o(std::filesystem::path(argv[2]) / name, std::ios::binary);
    o.write(reinterpret_cast<const char*>(out), len);
    if (!o) return 5;
    delete[] out;
    delete[] in;
  }
  delete state;
  return 0;
}
