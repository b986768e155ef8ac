// The C++ mirror's apply_pauli_sum, pauli_matrix_elements and inner (rustqip_amd/host/qip_hip.hpp over include/qip_hipx.h) on two
// states read from files.  Built and run by tests/test_gpu_f2_pauli_pair.py, which compares with Python's, bit for bit.
//   test_pair_mirror <n> <a: 2^n complex doubles> <b: the same> <out> (<string of n characters over IXYZ> <re> <im>)...
// (re, im as hexadecimal floats).  Writes to <out>, as complex doubles: b + H a (2^n), then <a| P_t |b> for every term, then <a|b>.
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
  if (argc < 8 || (argc - 5) % 3) {
    std::fprintf(stderr, "usage: %s n a.bin b.bin out.bin (string re im)...\n", argv[0]);
    return 2;
  }
  try {
    const size_t n = (size_t)std::atoi(argv[1]);
    const auto a = read_all<std::complex<double>>(argv[2]), b = read_all<std::complex<double>>(argv[3]);
    if (a.size() != (size_t(1) << n) || b.size() != a.size()) throw std::runtime_error("a state file does not hold 2^n amplitudes");
    std::vector<std::vector<std::pair<size_t, int>>> terms;
    std::vector<std::complex<double>> coeffs;
    for (int i = 5; i < argc; i += 3) {
      if (std::strlen(argv[i]) != n) throw std::runtime_error("a string does not have n characters");
      std::vector<std::pair<size_t, int>> term;
      for (size_t qb = 0; qb < n; ++qb) {
        const char* at = std::strchr(kCodes, argv[i][qb]);
        if (!at || !*at) throw std::runtime_error("a character that is none of IXYZ");
        if (*at != 'I') term.push_back({qb, int(at - kCodes)});
      }
      terms.push_back(term);
      coeffs.push_back({std::strtod(argv[i + 1], nullptr), std::strtod(argv[i + 2], nullptr)});
    }
    qip::HipState<double> sa(n), sb(n), sum(n);
    sa.upload(a);
    sb.upload(b);
    const auto elements = sa.pauli_matrix_elements(sb, terms);
    const auto inner = sa.inner(sb);
    sum.upload(b);
    sum.apply_pauli_sum(sa, terms, coeffs, true);
    auto out_amps = sum.download();
    // not accumulating into a zero state is accumulating minus the rounding of 0 + p: check the plain form against b = 0
    sum.apply_pauli_sum(sa, terms, coeffs);
    const auto plain = sum.download();
    sb.apply_pauli_sum(sa, {}, {});  // no terms: sb <- 0
    sb.apply_pauli_sum(sa, terms, coeffs, true);
    const auto onto_zero = sb.download();
    for (size_t j = 0; j < plain.size(); ++j)
      if (!(plain[j] == onto_zero[j])) throw std::runtime_error("the sum onto a zeroed state differs from the plain sum");
    bool refused = false;
    try {
      sum.apply_pauli_sum(sa, terms, {{0.5, 0.0}});
    } catch (const std::invalid_argument&) {
      refused = true;
    }
    if (!refused && terms.size() != 1) throw std::runtime_error("a coefficient list of another length was accepted");
    refused = false;
    try {
      sum.apply_pauli_sum(sum, terms, coeffs);
    } catch (const std::exception&) {
      refused = true;
    }
    if (!refused) throw std::runtime_error("the destination was accepted as the source");
    out_amps.insert(out_amps.end(), elements.begin(), elements.end());
    out_amps.push_back(inner);
    std::ofstream out(argv[4], std::ios::binary);
    out.write(reinterpret_cast<const char*>(out_amps.data()), (std::streamsize)(out_amps.size() * sizeof(out_amps[0])));
    if (!out) throw std::runtime_error("cannot write the result");
  } catch (const std::exception& e) {
    std::fprintf(stderr, "FAILED: %s\n", e.what());
    return 1;
  }
  return 0;
}
