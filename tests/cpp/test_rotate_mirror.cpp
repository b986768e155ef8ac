// The C++ mirror's apply_pauli_rotations (rustqip_amd/host/qip_hip.hpp over include/qip_hipx.h) on a state read from a file:
// writes the rotated state to a file.  Built and run by tests/test_gpu_f1_pauli_rotation.py, which compares with Python's.
//   test_rotate_mirror <n> <state: 2^n complex doubles> <out> (<string of n characters over IXYZ> <angle as a hexadecimal float>)...
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
  if (argc < 6 || (argc - 4) % 2) {
    std::fprintf(stderr, "usage: %s n state.bin out.bin (string angle)...\n", argv[0]);
    return 2;
  }
  try {
    const size_t n = (size_t)std::atoi(argv[1]);
    const auto amps = read_all<std::complex<double>>(argv[2]);
    if (amps.size() != (size_t(1) << n)) throw std::runtime_error("state file does not hold 2^n amplitudes");
    std::vector<std::vector<std::pair<size_t, int>>> terms;
    std::vector<double> angles;
    for (int i = 4; i < argc; i += 2) {
      if (std::strlen(argv[i]) != n) throw std::runtime_error("a string does not have n characters");
      std::vector<std::pair<size_t, int>> term;
      for (size_t qb = 0; qb < n; ++qb) {
        const char* at = std::strchr(kCodes, argv[i][qb]);
        if (!at || !*at) throw std::runtime_error("a character that is none of IXYZ");
        if (*at != 'I') term.push_back({qb, int(at - kCodes)});
      }
      terms.push_back(term);
      angles.push_back(std::strtod(argv[i + 1], nullptr));
    }
    qip::HipState<double> st(n);
    st.upload(amps);
    st.apply_pauli_rotations(terms, angles);
    const auto batch = st.download();
    // the single-term calls leave the same bits
    st.upload(amps);
    for (size_t t = 0; t < terms.size(); ++t) st.apply_pauli_rotations({terms[t]}, {angles[t]});
    const auto singles = st.download();
    if (std::memcmp(batch.data(), singles.data(), batch.size() * sizeof(batch[0])) != 0)
      throw std::runtime_error("the single-term calls differ from the batch");
    bool refused = false;
    try {
      st.apply_pauli_rotations(terms, {0.5});
    } catch (const std::invalid_argument&) {
      refused = true;
    }
    if (!refused && terms.size() != 1) throw std::runtime_error("an angle list of another length was accepted");
    std::ofstream out(argv[3], std::ios::binary);
    out.write(reinterpret_cast<const char*>(batch.data()), (std::streamsize)(batch.size() * sizeof(batch[0])));
    if (!out) throw std::runtime_error("cannot write the result");
  } catch (const std::exception& e) {
    std::fprintf(stderr, "FAILED: %s\n", e.what());
    return 1;
  }
  return 0;
}
