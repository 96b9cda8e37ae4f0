// dump_fmt_check.cc — the line arithmetic of task = dump (csrc/dfh_dumptext_fmt.h over csrc/dfh_predtext_fmt.h) compiled for
// the host and compared with the C library: whole lines "<id>\t<w>[\t<V_j>]\n" against snprintf("%llu"), ("\t%.9g"), byte for
// byte.  Built with -fsanitize=address,undefined by tests/test_dump_fmt_host.py; every line is assembled in a heap block of
// exactly dt_max_line(V_dim) bytes, so a byte placed outside a line is a report.
//   usage: dump_fmt_check [random bit patterns, default 100000]
// Prints one summary line and returns 0, or the first mismatches and 1.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "dfh_dumptext_fmt.h"

namespace {
int g_bad = 0;
uint64_t g_lines = 0, g_values = 0, g_irregular = 0;

uint32_t Bits(float v) {
  uint32_t b;
  memcpy(&b, &v, 4);
  return b;
}
float Float(uint32_t b) {
  float v;
  memcpy(&v, &b, 4);
  return v;
}
// the definition, not the formatter's test: +-0 and the finite v with 2^-64 <= |v| < 2^32
bool Regular(float v) { return v == 0.f || (std::isfinite(v) && std::fabs(v) >= std::ldexp(1.0f, -64) && std::fabs(v) < std::ldexp(1.0f, 32)); }

std::string Oracle(uint64_t id, float w, bool has_V, const float* V, uint32_t V_dim) {
  char buf[64];
  std::string s(buf, (size_t)snprintf(buf, sizeof(buf), "%llu", (unsigned long long)id));
  s.append(buf, (size_t)snprintf(buf, sizeof(buf), "\t%.9g", w));
  for (uint32_t j = 0; has_V && j < V_dim; ++j) s.append(buf, (size_t)snprintf(buf, sizeof(buf), "\t%.9g", V[j]));
  s.push_back('\n');
  return s;
}

// one line of regular values: equal to the oracle, nothing irregular
void CheckLine(uint64_t id, float w, bool has_V, const std::vector<float>& V) {
  const uint32_t V_dim = (uint32_t)V.size();
  std::vector<uint32_t> vb(V_dim ? V_dim : 1);
  for (uint32_t j = 0; j < V_dim; ++j) vb[j] = Bits(V[j]);
  const size_t room = (size_t)dfh_dt::dt_max_line(V_dim);
  unsigned char* dst = (unsigned char*)malloc(room);
  uint32_t irregular = 0;
  const uint32_t len = dfh_dt::dt_line(dst, id, Bits(w), has_V, vb.data(), V_dim, &irregular);
  const std::string want = Oracle(id, w, has_V, V.data(), V_dim);
  ++g_lines;
  g_values += 1 + (has_V ? V_dim : 0);
  if (irregular != 0 || len != want.size() || len > room || memcmp(dst, want.data(), len) != 0) {
    if (g_bad++ < 10)
      fprintf(stderr, "MISMATCH id=%llu V_dim=%u has_V=%d irregular=%u len=%u want %zu\n got  %.*s want %s", (unsigned long long)id, V_dim,
              (int)has_V, irregular, len, want.size(), (int)len, (const char*)dst, want.c_str());
  }
  free(dst);
}

// an irregular value is reported, not formatted: a field of length 0, and a line that counts it
void CheckIrregular(float v) {
  ++g_irregular;
  const dfh_dt::Field F = dfh_dt::dt_field(Bits(v));
  std::vector<uint32_t> vb(3, Bits(1.5f));
  vb[1] = Bits(v);
  unsigned char* dst = (unsigned char*)malloc((size_t)dfh_dt::dt_max_line(3));
  uint32_t irr_V = 0, irr_w = 0;
  const uint32_t len_V = dfh_dt::dt_line(dst, 77, Bits(0.25f), true, vb.data(), 3, &irr_V);
  const uint32_t len_w = dfh_dt::dt_line(dst, 77, Bits(v), false, vb.data(), 3, &irr_w);
  free(dst);
  // "77" "\t0.25" "\t1.5" (nothing) "\t1.5" "\n";  "77" (nothing) "\n"
  if (F.len != 0 || irr_V != 1 || irr_w != 1 || len_V != 2 + 5 + 4 + 4 + 1 || len_w != 3) {
    if (g_bad++ < 10) fprintf(stderr, "IRREGULAR %a (bits %08x): field %u, counted %u / %u, lines of %u / %u bytes\n", v, Bits(v), F.len, irr_V, irr_w, len_V, len_w);
  }
}

uint64_t g_rng = 0x9E3779B97F4A7C15ULL;
uint64_t Next() {   // splitmix64
  uint64_t z = (g_rng += 0x9E3779B97F4A7C15ULL);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}
}  // namespace

int main(int argc, char** argv) {
  const size_t n_random = argc > 1 ? (size_t)atoll(argv[1]) : 100000;
  // ids of every digit count 1 .. 20, at both ends of each
  std::vector<uint64_t> ids = {0, 1, 18446744073709551614ULL, 18446744073709551615ULL, 10000000000000000ULL - 1, 10000000000000000ULL,
                               100000000ULL - 1, 100000000ULL, 12345678901234567890ULL, 10000000100000000ULL};
  for (uint64_t p = 10, d = 1; d <= 19; ++d, p *= 10) {
    ids.push_back(p - 1);
    ids.push_back(p);
    if (d == 19) break;
  }
  bool seen[21] = {false};
  for (uint64_t id : ids) seen[dfh_dt::dt_id(id).nd] = true;
  for (int d = 1; d <= 20; ++d)
    if (!seen[d]) {
      fprintf(stderr, "no id of %d digits\n", d);
      return 1;
    }
  // designed values: +-0, exact ties, both ends of the regular range, both renderings around 1e-4 and 1e9
  std::vector<float> designed = {0.f, -0.f, 2097151.875f, 2097151.625f, 2097151.375f, 1048575.9375f, 0.5f, 16.f, 1e8f, 1e9f, 123456792.f,
                                 999999936.f, 4294967040.f, std::ldexp(1.0f, -64), std::nextafter(std::ldexp(1.0f, -64), 1.0f), 1e-4f,
                                 std::nextafter(1e-4f, 1.0f), 0.001f, 20.f, -1.23456789e-5f, std::nextafter(std::ldexp(1.0f, 32), 0.f)};
  for (size_t i = 0, n = designed.size(); i < n; ++i) designed.push_back(-designed[i]);
  for (float v : designed)
    if (!Regular(v)) {
      fprintf(stderr, "designed value %a is not regular\n", v);
      return 1;
    }
  // random bit patterns: the regular ones fill lines, the others must be reported
  std::vector<float> regular;
  for (size_t i = 0; i < n_random; ++i) {
    const float v = Float((uint32_t)Next());
    if (Regular(v)) regular.push_back(v); else CheckIrregular(v);
  }
  for (float v : {NAN, -NAN, INFINITY, -INFINITY, Float(1), Float(0x007FFFFF), Float(0x80000001), std::ldexp(1.0f, -70),
                  std::nextafter(std::ldexp(1.0f, -64), 0.f), std::ldexp(1.0f, 32), std::ldexp(1.0f, 33), -std::ldexp(1.0f, 33), 3e38f})
    CheckIrregular(v);
  std::vector<float> pool = designed;
  pool.insert(pool.end(), regular.begin(), regular.end());
  size_t at = 0, id_at = 0;
  auto take = [&] { return pool[at++ % pool.size()]; };
  for (uint32_t V_dim : {0u, 1u, 64u}) {
    // every id with and without V; then lines until the whole pool has been through this V_dim once
    const size_t start = at;
    for (size_t i = 0; i < ids.size() || at - start < pool.size(); ++i) {
      std::vector<float> V(V_dim);
      const float w = take();
      for (auto& x : V) x = take();
      const uint64_t id = i < ids.size() ? ids[i] : (Next() >> (Next() % 64));
      CheckLine(id, w, true, V);
      CheckLine(ids[id_at++ % ids.size()], w, false, V);
    }
  }
  // the longest line: a 20-digit id and 16-byte fields throughout
  CheckLine(18446744073709551615ULL, -1.23456789e-5f, true, std::vector<float>(64, -1.23456789e-5f));
  {
    const std::string longest = Oracle(18446744073709551615ULL, -1.23456789e-5f, true, std::vector<float>(64, -1.23456789e-5f).data(), 64);
    if (longest.size() != dfh_dt::dt_max_line(64)) {
      fprintf(stderr, "the longest line has %zu bytes, dt_max_line(64) = %llu\n", longest.size(), (unsigned long long)dfh_dt::dt_max_line(64));
      return 1;
    }
  }
  if (g_bad) {
    fprintf(stderr, "%d mismatches\n", g_bad);
    return 1;
  }
  printf("ok: %llu lines, %llu values, %llu irregular values reported, %zu random bit patterns\n", (unsigned long long)g_lines,
         (unsigned long long)g_values, (unsigned long long)g_irregular, n_random);
  return 0;
}
