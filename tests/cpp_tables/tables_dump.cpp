// tests/cpp_tables/tables_dump.cpp -- writes what nfllib_amd/csrc/host_tables.cpp computes to stdout, for
// tests/test_host_tables_cpu.py.  Host code only: built with g++ from this file and host_tables.cpp, no HIP, no library.
//   tables_dump tables <limb_bits> <n> <nm> <cyclic> <kmax_log2>     stdin: nm lines "P root invk" (decimal)
//   tables_dump reftab <limb_bits> <n> <kmax_log2> <which> <p> <phi> <invk>
// Output: records "<name> <nbytes>\n" followed by nbytes raw bytes.  `tables`: rc (int64) first and, when it is not 0, error (the
// message) and nothing else; then the 16 device tables (0 bytes: absent), the scalars and shape facts as 8-byte integers,
// inv_qtop (the double's 8 bytes), h_Q, h_lifting ([count, limbs...] per modulus) and h_phi as 64-bit words.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../nfllib_amd/csrc/host_tables.h"

using nflhip::HostTables;

static void put(const char *name, const void *data, size_t bytes) {
  std::printf("%s %zu\n", name, bytes);
  if (bytes) std::fwrite(data, 1, bytes, stdout);
}
static void put(const char *name, const HostTables::Bytes &b) { put(name, b.data(), b.size()); }
static void put(const char *name, const std::vector<uint64_t> &v) { put(name, v.data(), v.size() * 8); }
static void put_int(const char *name, int64_t v) { put(name, &v, 8); }

static int dump_tables(int limb_bits, size_t n, size_t nm, int cyclic, int kmax_log2) {
  std::vector<uint64_t> in(3 * nm);
  for (uint64_t &v : in)
    if (std::scanf("%llu", (unsigned long long *)&v) != 1) return 2;
  std::vector<unsigned char> par[3];  // P, roots, invk as arrays of limbs
  const size_t w = (size_t)limb_bits / 8;
  for (int k = 0; k < 3; ++k) {
    par[k].resize(nm * w);
    for (size_t cm = 0; cm < nm; ++cm) std::memcpy(&par[k][cm * w], &in[3 * cm + k], w);  // (little-endian host)
  }
  HostTables h;
  std::string err;
  const int rc = nflhip::build_host_tables(limb_bits, n, nm, cyclic, kmax_log2, par[0].data(), par[1].data(), par[2].data(), &h, &err);
  put_int("rc", rc);
  if (rc) {
    put("error", err.data(), err.size());
    return 0;
  }
  put("psi", h.psi);
  put("psi_lm", h.psi_lm);
  put("mc", h.mc);
  put("mc_inc0", h.mc_inc[0]);
  put("mc_inc1", h.mc_inc[1]);
  put("resc", h.resc);
  put("qhat", h.qhat);
  put("qsh", h.qsh);
  put("qparts", h.qparts);
  put("bparts", h.bparts);
  put("qhat_w", h.qhat_w);
  put("qsh_w", h.qsh_w);
  put("crt_bfrag", h.crt_bfrag);
  put("crt_bproj", h.crt_bproj);
  put("crt_coff", h.crt_coff);
  put("crt_c2048", h.crt_c2048);
  put_int("proj_K", h.proj_K);
  put_int("crt_Lw", h.crt_Lw);
  put_int("crt_nsh", h.crt_nsh);
  put_int("crt_L", (int64_t)h.crt_L);
  put_int("crt_Lacc", (int64_t)h.crt_Lacc);
  put_int("crt_Q0", (int64_t)h.crt_Q0);
  put_int("small_delta", h.small_delta);
  put_int("nm_small", h.nm_small);
  put("inv_qtop", &h.inv_qtop, 8);
  put("h_Q", h.Q);
  std::vector<uint64_t> lift;
  for (const std::vector<uint64_t> &l : h.lifting) {
    lift.push_back(l.size());
    lift.insert(lift.end(), l.begin(), l.end());
  }
  put("h_lifting", lift);
  put("h_phi", h.phi);
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 7 && !std::strcmp(argv[1], "tables"))
    return dump_tables(std::atoi(argv[2]), std::strtoull(argv[3], nullptr, 10), std::strtoull(argv[4], nullptr, 10), std::atoi(argv[5]),
                       std::atoi(argv[6]));
  if (argc == 9 && !std::strcmp(argv[1], "reftab")) {
    put("table", nflhip::reference_table(std::strtoull(argv[6], nullptr, 10), std::strtoull(argv[7], nullptr, 10),
                                         std::strtoull(argv[8], nullptr, 10), std::atoi(argv[4]), std::strtoull(argv[3], nullptr, 10),
                                         std::atoi(argv[2]), std::atoi(argv[5])));
    return 0;
  }
  std::fprintf(stderr, "usage: see the head of tables_dump.cpp\n");
  return 2;
}
