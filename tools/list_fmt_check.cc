// list_fmt_check.cc — the line arithmetic of explain_out and recommend_out (csrc/dfh_listtext_fmt.h over csrc/dfh_dumptext_fmt.h
// and csrc/dfh_predtext_fmt.h) compiled for the host and compared with the C library: whole lines against the learner's
// snprintf("%.9g"), ("\t%llu:%llu:%.9g") and ("%s%u:%.9g"), byte for byte.  Built with -fsanitize=address,undefined by
// tests/test_list_fmt_host.py; every line is assembled in a heap block of exactly lt_*_max_line(K) bytes, so a byte placed
// outside a line is a report.
//   usage: list_fmt_check [random lines per kind, default 20000]
// Prints one summary line and returns 0, or the first mismatches and 1.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "dfh_listtext_fmt.h"

namespace {
int g_bad = 0;
uint64_t g_lines = 0, g_entries = 0;

uint32_t Bits(float v) {
  uint32_t b;
  memcpy(&b, &v, 4);
  return b;
}

std::string ExplainOracle(float inter, const std::vector<uint64_t>& a, const std::vector<uint64_t>& b, const std::vector<float>& c) {
  char buf[96];
  std::string s(buf, (size_t)snprintf(buf, sizeof(buf), "%.9g", inter));
  for (size_t j = 0; j < c.size(); ++j)
    s.append(buf, (size_t)snprintf(buf, sizeof(buf), "\t%llu:%llu:%.9g", (unsigned long long)a[j], (unsigned long long)b[j], c[j]));
  s.push_back('\n');
  return s;
}

std::string RecommendOracle(const std::vector<uint32_t>& items, const std::vector<float>& logits) {
  char buf[64];
  std::string s;
  for (size_t j = 0; j < items.size(); ++j) s.append(buf, (size_t)snprintf(buf, sizeof(buf), "%s%u:%.9g", j ? "\t" : "", items[j], logits[j]));
  s.push_back('\n');
  return s;
}

void Compare(const char* kind, size_t K, const unsigned char* dst, uint32_t len, uint32_t irregular, size_t room, const std::string& want) {
  ++g_lines;
  if (irregular != 0 || len != want.size() || len > room || memcmp(dst, want.data(), len) != 0) {
    if (g_bad++ < 10)
      fprintf(stderr, "MISMATCH %s K=%zu irregular=%u len=%u want %zu\n got  %.*s want %s", kind, K, irregular, len, want.size(), (int)len,
              (const char*)dst, want.c_str());
  }
}

// a line of n entries in the room of K
void CheckExplain(size_t K, float inter, const std::vector<uint64_t>& a, const std::vector<uint64_t>& b, const std::vector<float>& c) {
  std::vector<uint32_t> cb(c.size() ? c.size() : 1);
  for (size_t j = 0; j < c.size(); ++j) cb[j] = Bits(c[j]);
  const size_t room = (size_t)dfh_lt::lt_explain_max_line(K);
  unsigned char* dst = (unsigned char*)malloc(room);
  uint32_t irregular = 0;
  const uint32_t len = dfh_lt::lt_explain_line(dst, Bits(inter), (uint32_t)c.size(), a.data(), b.data(), cb.data(), &irregular);
  g_entries += c.size();
  Compare("explain", K, dst, len, irregular, room, ExplainOracle(inter, a, b, c));
  free(dst);
}

void CheckRecommend(size_t K, const std::vector<uint32_t>& items, const std::vector<float>& logits) {
  std::vector<uint32_t> lb(logits.size() ? logits.size() : 1);
  for (size_t j = 0; j < logits.size(); ++j) lb[j] = Bits(logits[j]);
  const size_t room = (size_t)dfh_lt::lt_recommend_max_line(K);
  unsigned char* dst = (unsigned char*)malloc(room);
  uint32_t irregular = 0;
  const uint32_t len = dfh_lt::lt_recommend_line(dst, (uint32_t)items.size(), items.data(), lb.data(), &irregular);
  g_entries += items.size();
  Compare("recommend", K, dst, len, irregular, room, RecommendOracle(items, logits));
  free(dst);
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
  const size_t n_random = argc > 1 ? (size_t)atoll(argv[1]) : 20000;
  // ids and items of every digit count, at both ends of each
  std::vector<uint64_t> ids = {0, 18446744073709551615ULL, 12345678901234567890ULL};
  std::vector<uint32_t> items = {0, 4294967295u, 2147483647u};
  for (uint64_t p = 10, d = 1; d <= 19; ++d, p *= 10) {
    ids.push_back(p - 1);
    ids.push_back(p);
    if (d <= 9) {
      items.push_back((uint32_t)(p - 1));
      items.push_back((uint32_t)p);
    }
    if (d == 19) break;
  }
  // floats: +-0, exact ties, both ends of the regular range, both renderings around 1e-4 and 1e9, the longest texts
  std::vector<float> vals = {0.f, -0.f, 2097151.875f, 2097151.625f, 0.5f, 16.f, 1e8f, 1e9f, 123456792.f, 999999936.f, 4294967040.f,
                             std::ldexp(1.0f, -64), 1e-4f, std::nextafter(1e-4f, 1.0f), 0.001f, 20.f, -1.23456789e-5f, -0.000123456789f,
                             std::nextafter(std::ldexp(1.0f, 32), 0.f), 3.14159274f};
  for (size_t i = 0, n = vals.size(); i < n; ++i) vals.push_back(-vals[i]);
  size_t va = 0, ia = 0, ta = 0;
  auto val = [&] { return vals[va++ % vals.size()]; };
  // every list length 0 .. K for K in {1, 10, 32}, the designed tokens going round
  for (size_t K : {1u, 10u, 32u})
    for (size_t rep = 0; rep < 8; ++rep)
      for (size_t n = 0; n <= K; ++n) {
        std::vector<uint64_t> a(n), b(n);
        std::vector<uint32_t> it(n);
        std::vector<float> c(n);
        for (size_t j = 0; j < n; ++j) {
          a[j] = ids[ia++ % ids.size()];
          b[j] = ids[(ia * 7 + j) % ids.size()];
          it[j] = items[ta++ % items.size()];
          c[j] = val();
        }
        CheckExplain(K, val(), a, b, c);
        CheckRecommend(K, it, c);
      }
  // the longest lines fill their room exactly (recommend's bound counts a tab the first entry does not have)
  {
    const size_t K = 32;
    std::vector<uint64_t> a(K, 18446744073709551615ULL);
    std::vector<uint32_t> it(K, 4294967295u);
    std::vector<float> c(K, -1.23456789e-5f);
    CheckExplain(K, -1.23456789e-5f, a, a, c);
    CheckRecommend(K, it, c);
    if (ExplainOracle(-1.23456789e-5f, a, a, c).size() != dfh_lt::lt_explain_max_line(K) ||
        RecommendOracle(it, c).size() + 1 != dfh_lt::lt_recommend_max_line(K)) {
      fprintf(stderr, "the longest lines do not have lt_explain_max_line / lt_recommend_max_line - 1 bytes\n");
      return 1;
    }
  }
  // random lines: regular floats from random bit patterns, ids of random width
  for (size_t i = 0; i < n_random; ++i) {
    const size_t K = 1 + Next() % 32, n = Next() % (K + 1);
    std::vector<uint64_t> a(n), b(n);
    std::vector<uint32_t> it(n);
    std::vector<float> c(n);
    auto regular = [&] {
      for (;;) {
        const uint32_t bits = (uint32_t)Next();
        if (dfh_pt::pt_format(bits).len) {
          float v;
          memcpy(&v, &bits, 4);
          return v;
        }
      }
    };
    for (size_t j = 0; j < n; ++j) {
      a[j] = Next() >> (Next() % 64);
      b[j] = Next() >> (Next() % 64);
      it[j] = (uint32_t)(Next() >> (32 + Next() % 32));
      c[j] = regular();
    }
    CheckExplain(K, regular(), a, b, c);
    CheckRecommend(K, it, c);
  }
  // a float outside the regular range is reported, not formatted
  for (float v : {NAN, INFINITY, -INFINITY, 1e-12f * 1e-12f, std::ldexp(1.0f, 32), -3e38f}) {
    const uint64_t a[2] = {7, 8};
    const uint32_t it[2] = {7, 8}, cb[2] = {Bits(1.5f), Bits(v)};
    unsigned char* dst = (unsigned char*)malloc((size_t)dfh_lt::lt_explain_max_line(2));
    uint32_t i0 = 0, i1 = 0, i2 = 0;
    dfh_lt::lt_explain_line(dst, Bits(v), 0, a, a, cb, &i0);
    dfh_lt::lt_explain_line(dst, Bits(0.25f), 2, a, a, cb, &i1);
    dfh_lt::lt_recommend_line(dst, 2, it, cb, &i2);
    free(dst);
    if (i0 != 1 || i1 != 1 || i2 != 1) {
      if (g_bad++ < 10) fprintf(stderr, "IRREGULAR %a: counted %u / %u / %u\n", v, i0, i1, i2);
    }
  }
  if (g_bad) {
    fprintf(stderr, "%d mismatches\n", g_bad);
    return 1;
  }
  printf("ok: %llu lines, %llu entries, %zu random lines per kind\n", (unsigned long long)g_lines, (unsigned long long)g_entries, n_random);
  return 0;
}
