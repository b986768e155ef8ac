// The C++ mirror's linear_combination and inner_products (rustqip_amd/host/qip_hip.hpp over include/qip_hipx.h) on three states
// read from files.  Built and run by tests/test_gpu_f3_krylov.py, which compares with Python's, bit for bit.
//   test_krylov_mirror <n> <a: 2^n complex doubles> <b: the same> <c: the same> <out> (<re> <im>) x 3
// (re, im as hexadecimal floats: the coefficients of a, b, c).  Writes to <out>, as complex doubles: k_a a + k_b b + k_c c (2^n),
// then (its squared norm, 0), then <a|c>, <b|c>, <c|c>, then b after b <- k_b b + k_a a in place (2^n).
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
  if (argc != 12) {
    std::fprintf(stderr, "usage: %s n a.bin b.bin c.bin out.bin re im re im re im\n", argv[0]);
    return 2;
  }
  try {
    const size_t n = (size_t)std::atoi(argv[1]);
    const auto a = read_all<std::complex<double>>(argv[2]), b = read_all<std::complex<double>>(argv[3]),
               c = read_all<std::complex<double>>(argv[4]);
    if (a.size() != (size_t(1) << n) || b.size() != a.size() || c.size() != a.size())
      throw std::runtime_error("a state file does not hold 2^n amplitudes");
    std::vector<std::complex<double>> k;
    for (int i = 6; i < 12; i += 2) k.push_back({std::strtod(argv[i], nullptr), std::strtod(argv[i + 1], nullptr)});
    qip::HipState<double> sa(n), sb(n), sc(n), dst(n);
    sa.upload(a);
    sb.upload(b);
    sc.upload(c);
    double norm = -1.0;
    dst.linear_combination({&sa, &sb, &sc}, k, &norm);
    auto out = dst.download();
    out.push_back({norm, 0.0});
    const auto inner = sc.inner_products({&sa, &sb, &sc});
    out.insert(out.end(), inner.begin(), inner.end());
    sb.linear_combination({&sb, &sa}, {k[1], k[0]});
    const auto scaled = sb.download();
    out.insert(out.end(), scaled.begin(), scaled.end());
    // no sources: zero, and a norm of zero
    norm = -1.0;
    dst.linear_combination({}, {}, &norm);
    for (const auto& v : dst.download())
      if (v != std::complex<double>(0.0, 0.0)) throw std::runtime_error("no sources did not leave zero");
    if (norm != 0.0) throw std::runtime_error("no sources did not return a norm of zero");
    bool refused = false;
    try {
      dst.linear_combination({&sa, &sb}, {k[0]});
    } catch (const std::invalid_argument&) {
      refused = true;
    }
    if (!refused) throw std::runtime_error("a coefficient list of another length was accepted");
    refused = false;
    try {
      dst.linear_combination(std::vector<qip::HipState<double>*>(17, &sa), std::vector<std::complex<double>>(17, k[0]));
    } catch (const std::exception&) {
      refused = true;
    }
    if (!refused) throw std::runtime_error("seventeen sources were accepted");
    std::ofstream f(argv[5], std::ios::binary);
    f.write(reinterpret_cast<const char*>(out.data()), (std::streamsize)(out.size() * sizeof(out[0])));
    if (!f) throw std::runtime_error("cannot write the result");
  } catch (const std::exception& e) {
    std::fprintf(stderr, "FAILED: %s\n", e.what());
    return 1;
  }
  return 0;
}
