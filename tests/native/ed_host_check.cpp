// Test infrastructure: runs the kernels' Ed25519 code (ed25519_core.hpp) on the host so
// tests/test_ed25519.py can check the arithmetic against the oracle without a GPU.  Not
// part of the library.  stdin lines: "pk SEED" | "sign SEED MSG" | "verify PK MSG SIG"
// (hex, MSG may be "-" for empty); stdout: one hex / 0 / 1 line each.  "bench_verify PK MSG
// SIG N" times N verifications on one host thread (bench_sig.py's native CPU baseline leg)
// and prints verifications per second.
//
// Field ops on explicit limb vectors (ten signed decimal integers per operand, limb i at bit
// kOff[i]): "fe_mul F G" | "fe_sq F" | "fe_sq2 F" | "fe_invert F" print the result's ten limbs
// as one comma-separated token; "fe_to_words F" prints the canonical value's 32 bytes (hex).
// They reach limb patterns at the header's bound rule, which no signature is known to produce.
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "ed25519_core.hpp"

using namespace ag::ed;

static std::vector<uint8_t> unhex(const std::string& s) {
  std::vector<uint8_t> v;
  if (s == "-") return v;
  for (size_t i = 0; i + 1 < s.size(); i += 2) v.push_back(static_cast<uint8_t>(std::stoi(s.substr(i, 2), nullptr, 16)));
  return v;
}
static std::string hex(const uint8_t* p, size_t n) {
  static const char* d = "0123456789abcdef";
  std::string s;
  for (size_t i = 0; i < n; ++i) {
    s += d[p[i] >> 4];
    s += d[p[i] & 15];
  }
  return s;
}

static bool read_fe(std::istringstream& is, Fe& f) {
  for (int i = 0; i < 10; ++i) {
    long long v;
    if (!(is >> v) || v < INT32_MIN || v > INT32_MAX) return false;
    f.v[i] = static_cast<int32_t>(v);
  }
  return true;
}
static void print_fe(const Fe& f) {
  for (int i = 0; i < 10; ++i) std::cout << f.v[i] << (i < 9 ? "," : "\n");
}

int main() {
  std::vector<int32_t> table(64 * 8 * 30);
  for (int r = 0; r < 64; ++r) base_table_row(r, table.data());
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream is(line);
    std::string op, a, b, c;
    is >> op;
    if (op.rfind("fe_", 0) == 0) {
      Fe f, g, o;
      if (!read_fe(is, f) || (op == "fe_mul" && !read_fe(is, g))) {
        std::cout << "bad\n";
      } else if (op == "fe_to_words") {
        uint32_t w[8];
        uint8_t bytes[32];
        fe_to_words(f, w);
        store_words(bytes, w);
        std::cout << hex(bytes, 32) << "\n";
      } else {
        if (op == "fe_mul") fe_mul(o, f, g);
        else if (op == "fe_sq") fe_sq(o, f);
        else if (op == "fe_sq2") fe_sq2(o, f);
        else if (op == "fe_invert") fe_invert(o, f);
        else o = fe_zero();
        print_fe(o);
      }
      continue;
    }
    is >> a >> b >> c;
    if (op == "pk") {
      auto seed = unhex(a);
      uint8_t pk[32];
      public_key(seed.data(), pk, table.data());
      std::cout << hex(pk, 32) << "\n";
    } else if (op == "sign") {
      auto seed = unhex(a), msg = unhex(b);
      uint8_t pk[32], sig[64];
      public_key(seed.data(), pk, table.data());
      sign(seed.data(), pk, static_cast<uint32_t>(msg.size()), [&](uint32_t i) -> uint32_t { return msg[i]; }, sig,
           table.data());
      std::cout << hex(sig, 64) << "\n";
    } else if (op == "bench_verify") {
      auto pk = unhex(a), msg = unhex(b), sig = unhex(c);
      long n = 0;
      is >> n;
      Cached tab[9];
      int good = 0;
      const auto t0 = std::chrono::steady_clock::now();
      for (long r = 0; r < n; ++r)
        good += verify(pk.data(), sig.data(), static_cast<uint32_t>(msg.size()),
                       [&](uint32_t i) -> uint32_t { return msg[i]; }, table.data(), tab);
      const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      std::cout << (good == n ? n / dt : -1.0) << "\n";
    } else if (op == "verify") {
      auto pk = unhex(a), msg = unhex(b), sig = unhex(c);
      Cached tab[9];
      const bool ok = verify(pk.data(), sig.data(), static_cast<uint32_t>(msg.size()),
                             [&](uint32_t i) -> uint32_t { return msg[i]; }, table.data(), tab);
      std::cout << (ok ? 1 : 0) << "\n";
    }
  }
  return 0;
}
