// tests/cpp_scale_round/record_main.cpp -- prints the record of build_scale_round_record (nfllib_amd/csrc/host_tables.cpp, pure host
// code) for tests/test_scale_round_cpu.py to compare with its definition on Python integers.  Compiled under
// -fsanitize=address,undefined.
// Usage: record <limb_bits> <ks> <t>   with "nm\np_0 ... p_{nm-1}\n" on stdin.  Output: "<rc> <error text>", then one word per line.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "../../nfllib_amd/csrc/host_tables.h"

int main(int argc, char **argv) {
  if (argc != 4) return 2;
  const int lb = std::atoi(argv[1]);
  const size_t ks = std::strtoull(argv[2], nullptr, 10);
  const uint64_t t = std::strtoull(argv[3], nullptr, 10);
  size_t nm = 0;
  std::cin >> nm;
  std::vector<uint64_t> P(nm);
  for (size_t i = 0; i < nm; ++i) std::cin >> P[i];
  std::vector<uint64_t> rec;
  std::string err;
  const int rc = nflhip::build_scale_round_record(lb, P, ks, t, &rec, &err);
  std::printf("%d %s\n", rc, err.c_str());
  if (rc == 0)
    for (uint64_t w : rec) std::printf("%llu\n", (unsigned long long)w);
  return 0;
}
