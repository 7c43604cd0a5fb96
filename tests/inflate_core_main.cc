// Host driver of csrc/inflate_core.h for tests/test_inflate_core_cpu.py: inflates every file of a directory
// (u32 isize, then the raw deflate payload), one block at a time, and prints "<name> <status> <crc32 hex>" per
// file in name order (the CRC of the output for status 0, else 0).  Payload, output and tables live in heap
// blocks of their exact sizes, so AddressSanitizer sees any access one byte outside them.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <filesystem>
#include <fstream>
#include <string>
#include <vector>

#include "inflate_core.h"

using namespace snvrag;

struct HostSink {
  uint8_t* out;
  void put(int64_t pos, uint8_t v) { out[pos] = v; }
  void stored(int64_t pos, const uint8_t* src, int n) {
    for (int i = 0; i < n; ++i) out[pos + i] = src[i];
  }
  void match(int64_t pos, int dist, int len) {
    const uint8_t* src = out + (pos - dist);
    for (int i = 0; i < len; ++i) out[pos + i] = src[i % dist];
  }
};

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::vector<std::string> names;
  for (const auto& e : std::filesystem::directory_iterator(argv[1])) names.push_back(e.path().string());
  std::sort(names.begin(), names.end());
  uint32_t* table = new uint32_t[256];
  for (uint32_t i = 0; i < 256; ++i) table[i] = infl_crc_table_entry(i);
  for (const std::string& name : names) {
    std::ifstream f(name, std::ios::binary);
    std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    if (raw.size() < 4) return 3;
    uint32_t isize;
    std::memcpy(&isize, raw.data(), 4);
    if (isize > (uint32_t)INFL_MAX_ISIZE) return 4;
    const int64_t in_len = (int64_t)raw.size() - 4;
    uint8_t* payload = new uint8_t[in_len];
    std::memcpy(payload, raw.data() + 4, (size_t)in_len);
    uint8_t* out = new uint8_t[isize];
    InflTables* t = new InflTables;
    HostSink sink{out};
    int64_t produced = 0;
    const int st = infl_block(payload, in_len, (int64_t)isize, *t, sink, &produced);
    uint32_t crc = 0;
    if (st == INFL_OK) {
      // in two halves joined by the x^(8n) shift, as the kernel joins its lanes' segments
      const int64_t h = isize / 2;
      const uint32_t a = infl_crc_raw(0xffffffffu, out, h, table), b = infl_crc_raw(0u, out + h, isize - h, table);
      crc = (infl_crc_mul(a, infl_crc_x8n(isize - h)) ^ b) ^ 0xffffffffu;
    }
    std::printf("%s %d %08x\n", std::filesystem::path(name).filename().string().c_str(), st, crc);
    delete t;
    delete[] out;
    delete[] payload;
  }
  delete[] table;
  return 0;
}
