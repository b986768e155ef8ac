// The C++ mirror's expect_pauli (rustqip_amd/host/qip_hip.hpp over include/qip_hipx.h) on a state read from a file: prints one
// value per line, as hexadecimal floats.  Built and run by tests/test_gpu_f1_expect_pauli.py, which compares with Python's.
//   test_expect_mirror <n> <state: 2^n complex doubles> <string of n characters over IXYZ>...
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <vector>

#include "qip_hip.hpp"

template <typename V> static std::vector<V> read_all(const char* path) {
  std::ifstream f(path, std::ios::binary | std::ios::ate);
  if (!f) throw std::runtime_error(std::string("cannot open ") + path);
  const std::streamsize bytes = f.tellg();
  f.seekg(0);
  std::vector<V> v((size_t)bytes / sizeof(V));
  f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(v.size() * sizeof(V)));
  return v;
}

static const char kCodes[] = "IXYZ";  // the position is the code of include/qip_hipx.h

int main(int argc, char** argv) {
  if (argc < 4) {
    std::fprintf(stderr, "usage: %s n state.bin string...\n", argv[0]);
    return 2;
  }
  try {
    const size_t n = (size_t)std::atoi(argv[1]);
    const auto amps = read_all<std::complex<double>>(argv[2]);
    if (amps.size() != (size_t(1) << n)) throw std::runtime_error("state file does not hold 2^n amplitudes");
    std::vector<std::vector<std::pair<size_t, int>>> terms;
    for (int i = 3; i < argc; ++i) {
      if (std::strlen(argv[i]) != n) throw std::runtime_error("a string does not have n characters");
      std::vector<std::pair<size_t, int>> term;
      for (size_t qb = 0; qb < n; ++qb) {
        const char* at = std::strchr(kCodes, argv[i][qb]);
        if (!at || !*at) throw std::runtime_error("a character that is none of IXYZ");
        if (*at != 'I') term.push_back({qb, int(at - kCodes)});
      }
      terms.push_back(term);
    }
    qip::HipState<double> st(n);
    st.upload(amps);
    const std::vector<double> values = st.expect_pauli(terms);
    if (values.size() != terms.size()) throw std::runtime_error("result length");
    // one term by itself is the same number
    if (st.expect_pauli({terms.back()})[0] != values.back()) throw std::runtime_error("a single term differs from the batch");
    for (double v : values) std::printf("%a\n", v);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "FAILED: %s\n", e.what());
    return 1;
  }
  return 0;
}
