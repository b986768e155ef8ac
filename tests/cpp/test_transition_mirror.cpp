// The C++ mirror's transition_matrix (rustqip_amd/host/qip_hip.hpp over include/qip_hipx.h) on two states read from files.
// Built and run by tests/test_gpu_f2_transition.py, which compares with Python's, bit for bit.
//   test_transition_mirror <n> <bra: 2^n complex doubles> <ket: the same> <out> <qubits, comma separated>...
// Writes to <out>, as complex doubles, the row-major matrices of the index lists one after the other.
#include <cstdio>
#include <cstdlib>
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

int main(int argc, char** argv) {
  if (argc < 6) {
    std::fprintf(stderr, "usage: %s n bra.bin ket.bin out.bin q,q,... [q,q,...]...\n", argv[0]);
    return 2;
  }
  try {
    const size_t n = (size_t)std::atoi(argv[1]);
    const auto x = read_all<std::complex<double>>(argv[2]);
    const auto y = read_all<std::complex<double>>(argv[3]);
    if (x.size() != (size_t(1) << n) || y.size() != x.size()) throw std::runtime_error("a state file does not hold 2^n amplitudes");
    qip::HipState<double> bra(n), ket(n);
    bra.upload(x);
    ket.upload(y);
    std::vector<std::complex<double>> all;
    for (int i = 5; i < argc; ++i) {
      std::vector<size_t> indices;
      for (const char* at = argv[i]; *at;) {
        char* end = nullptr;
        indices.push_back((size_t)std::strtoul(at, &end, 10));
        at = *end == ',' ? end + 1 : end;
      }
      const auto rho = bra.transition_matrix(ket, indices);
      if (rho.size() != (size_t(1) << (2 * indices.size()))) throw std::runtime_error("a matrix of another size");
      all.insert(all.end(), rho.begin(), rho.end());
    }
    bool refused = false;
    try {
      bra.transition_matrix(ket, {0, 1, 2, 3});
    } catch (const std::exception&) {
      refused = true;
    }
    if (!refused && n >= 4) throw std::runtime_error("four qubits were accepted");
    const auto after_bra = bra.download(), after_ket = ket.download();
    for (size_t j = 0; j < x.size(); ++j)
      if (!(after_bra[j] == x[j]) || !(after_ket[j] == y[j])) throw std::runtime_error("a state was changed");
    std::ofstream out(argv[4], std::ios::binary);
    out.write(reinterpret_cast<const char*>(all.data()), (std::streamsize)(all.size() * sizeof(all[0])));
    if (!out) throw std::runtime_error("cannot write the result");
  } catch (const std::exception& e) {
    std::fprintf(stderr, "FAILED: %s\n", e.what());
    return 1;
  }
  return 0;
}
