// The C++ mirror's apply_diagonal and expect_diagonal (rustqip_amd/host/qip_hip.hpp over include/qip_hipx.h) on a state read from
// a file: prints the two moments of the state as read (17 significant digits) and writes the phased state to a file.  Built and
// run by tests/test_gpu_f2_diagonal.py, which compares with Python's.
//   test_diag_mirror <n> <state: 2^n complex doubles> <out> <gamma> (<string of n characters over IZ> <coefficient>)...
// (gamma and the coefficients as hexadecimal floats)
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
  if (argc < 7 || (argc - 5) % 2) {
    std::fprintf(stderr, "usage: %s n state.bin out.bin gamma (string coefficient)...\n", argv[0]);
    return 2;
  }
  try {
    const size_t n = (size_t)std::atoi(argv[1]);
    const auto amps = read_all<std::complex<double>>(argv[2]);
    if (amps.size() != (size_t(1) << n)) throw std::runtime_error("state file does not hold 2^n amplitudes");
    const double gamma = std::strtod(argv[4], nullptr);
    std::vector<std::vector<std::pair<size_t, int>>> terms;
    std::vector<double> coeffs;
    for (int i = 5; i < argc; i += 2) {
      if (std::strlen(argv[i]) != n) throw std::runtime_error("a string does not have n characters");
      std::vector<std::pair<size_t, int>> term;
      for (size_t qb = 0; qb < n; ++qb) {
        const char* at = std::strchr(kCodes, argv[i][qb]);
        if (!at || !*at) throw std::runtime_error("a character that is none of IXYZ");
        if (*at != 'I') term.push_back({qb, int(at - kCodes)});
      }
      terms.push_back(term);
      coeffs.push_back(std::strtod(argv[i + 1], nullptr));
    }
    qip::HipState<double> st(n);
    st.upload(amps);
    const auto moments = st.expect_diagonal(terms, coeffs);
    std::printf("%.17g %.17g\n", moments.first, moments.second);
    st.apply_diagonal(terms, coeffs, gamma);
    const auto phased = st.download();
    bool refused = false;
    try {
      st.apply_diagonal(terms, {0.5}, gamma);
    } catch (const std::invalid_argument&) {
      refused = true;
    }
    if (!refused && terms.size() != 1) throw std::runtime_error("a coefficient list of another length was accepted");
    refused = false;
    try {
      st.apply_diagonal({{{0, 1}}}, {0.5}, gamma);  // an X factor
    } catch (const std::exception&) {
      refused = true;
    }
    if (!refused) throw std::runtime_error("a term with an X factor was accepted");
    std::ofstream out(argv[3], std::ios::binary);
    out.write(reinterpret_cast<const char*>(phased.data()), (std::streamsize)(phased.size() * sizeof(phased[0])));
    if (!out) throw std::runtime_error("cannot write the result");
  } catch (const std::exception& e) {
    std::fprintf(stderr, "FAILED: %s\n", e.what());
    return 1;
  }
  return 0;
}
