// The C++ mirror's soft_measure_many (rustqip_amd/host/qip_hip.hpp over include/qip_hipx.h) on a state and samples read from
// files: prints one outcome per line.  Built and run by tests/test_gpu_f1_sample_many.py, which compares with Python's.
//   test_sample_mirror <n> <state: 2^n complex doubles> <samples: doubles> <qubit>...
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
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
  if (argc < 5) {
    std::fprintf(stderr, "usage: %s n state.bin samples.bin qubit...\n", argv[0]);
    return 2;
  }
  try {
    const size_t n = (size_t)std::atoi(argv[1]);
    const auto amps = read_all<std::complex<double>>(argv[2]);
    const auto samples = read_all<double>(argv[3]);
    std::vector<size_t> indices;
    for (int i = 4; i < argc; ++i) indices.push_back((size_t)std::atoi(argv[i]));
    if (amps.size() != (size_t(1) << n)) throw std::runtime_error("state file does not hold 2^n amplitudes");
    qip::HipState<double> st(n);
    st.upload(amps);
    const std::vector<uint64_t> many = st.soft_measure_many(indices, samples);
    if (many.size() != samples.size()) throw std::runtime_error("result length");
    // the mirror's single call on the first few samples: the two agree inside the mirror as well
    for (size_t j = 0; j < samples.size() && j < 8; ++j)
      if (st.soft_measure(indices, samples[j]) != many[j]) throw std::runtime_error("soft_measure_many differs from soft_measure");
    for (uint64_t m : many) std::cout << m << "\n";
  } catch (const std::exception& e) {
    std::fprintf(stderr, "FAILED: %s\n", e.what());
    return 1;
  }
  return 0;
}
