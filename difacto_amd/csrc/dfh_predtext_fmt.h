// dfh_predtext_fmt.h — the line fprintf("%.9g\n", v) writes for a float v, in exact integer arithmetic (the device formatter of
// dfh_predtext.hip; plain C++, so a host program can compile the same function and compare it with the C library).
//
// REGULAR values only: +0, -0, and the finite v with 2^-64 <= |v| < 2^32 (biased exponent 63..158).  Everything else — tiny,
// huge, subnormal, non-finite — gives a line of length 0 and is left to the host.
//
//   v = m 2^e, 2^23 <= m < 2^24, -87 <= e <= 8.
//   |v| >= 10^9 (exactly the float 1e9f and above): v is an integer N < 2^32 of ten digits, k = 9, and the nine digits are
//       N / 10 rounded half to even on N mod 10 (one 32-bit division; at most 429 496 704, so no carry into a tenth digit).
//   else k = floor(log10 |v|) is estimated from the binary exponent b = e + 23 as floor(b 78913 / 2^18) (78913 / 2^18 =
//       0.3010292 < log10 2, |b| <= 64: the estimate is k or k - 1, never above k), and the nine digits are
//           D = round-half-even(m 10^(8-k) 2^e).
//       8 - k <= 28, and 29 with an estimate one short: m 10^29 < 2^24 2^96.4 < 2^121, so an unsigned __int128 holds the product.
//       10^q comes from a table of 10^0 .. 10^19 (64-bit words), as 10^min(q,19) 10^(q - min(q,19)).  e < 0: the integer part is
//       the product shifted right by -e, and the shifted-out bits against the half decide the rounding, ties to even.  An
//       integer part >= 10^9 says the estimate was one short: once more with k + 1 (the digits are rounded only at the right k).
//       D = 10^9 after rounding is 1.00000000 at k + 1.
//   No division of the wide word, no floating point.
//   Rendering is %g's with precision 9: scientific when the ROUNDED exponent k < -4 or k >= 9 (two exponent digits and a sign:
//   |k| <= 20), else fixed; trailing zeros go, and the point with them when nothing follows it.  The longest lines have 16 bytes
//   with their '\n': -1.23456789e-05 and -0.000123456789.
#ifndef DFH_PREDTEXT_FMT_H_
#define DFH_PREDTEXT_FMT_H_
#include <stdint.h>

#if defined(__HIPCC__)
#define DFH_PT_FN __host__ __device__ __forceinline__
#else
#define DFH_PT_FN inline
#endif

namespace dfh_pt {

typedef unsigned __int128 u128;

struct Line {
  uint64_t lo, hi;   // the bytes of the line, the first in the lowest byte of lo
  uint32_t len;      // 2 .. 16 with the '\n'; 0: the value is not regular
};

constexpr uint32_t PT_MAX_LINE = 16;

// the integer part of m 10^q 2^e (0 <= q <= 29, -87 <= e <= 6) and whether round-half-even takes it one up
DFH_PT_FN uint64_t pt_scaled(uint32_t m, int e, uint32_t q, bool* up) {
  static constexpr uint64_t P10[20] = {1ULL, 10ULL, 100ULL, 1000ULL, 10000ULL, 100000ULL, 1000000ULL, 10000000ULL, 100000000ULL,
                                       1000000000ULL, 10000000000ULL, 100000000000ULL, 1000000000000ULL, 10000000000000ULL,
                                       100000000000000ULL, 1000000000000000ULL, 10000000000000000ULL, 100000000000000000ULL,
                                       1000000000000000000ULL, 10000000000000000000ULL};
  const uint32_t q1 = q < 19 ? q : 19;
  const u128 prod = (u128)P10[q1] * P10[q - q1] * m;
  if (e >= 0) {
    *up = false;
    return (uint64_t)(prod << e);
  }
  const uint32_t s = (uint32_t)-e;   // 1 .. 87
  const uint64_t ip = (uint64_t)(prod >> s);
  const u128 rem = prod & (((u128)1 << s) - 1), half = (u128)1 << (s - 1);
  *up = rem > half || (rem == half && (ip & 1));
  return ip;
}

DFH_PT_FN u128 pt_mask(uint32_t nbytes) { return (((u128)1 << (8 * nbytes - 1)) << 1) - 1; }   // 1 <= nbytes <= 16

DFH_PT_FN Line pt_format(uint32_t bits) {
  Line L;
  L.lo = L.hi = 0;
  L.len = 0;
  const uint32_t a = bits & 0x7FFFFFFFu, neg = bits >> 31, E = a >> 23;
  if (a == 0) {
    L.lo = neg ? ('-' | '0' << 8 | '\n' << 16) : ('0' | '\n' << 8);
    L.len = neg ? 3 : 2;
    return L;
  }
  if (E < 63 || E > 158) return L;
  const uint32_t m = (a & 0x7FFFFFu) | 0x800000u;
  const int e = (int)E - 150;
  uint32_t D;
  int k;
  if (a >= 0x4E6E6B28u) {   // 1e9f
    const uint32_t N = m << e, q = N / 10, r = N - q * 10;
    D = q + ((r > 5 || (r == 5 && (q & 1))) ? 1u : 0u);
    k = 9;
  } else {
    k = (((int)E - 127) * 78913) >> 18;   // the arithmetic shift is the floor
    bool up;
    uint64_t ip = pt_scaled(m, e, (uint32_t)(8 - k), &up);
    if (ip >= 1000000000ULL) {
      ++k;
      ip = pt_scaled(m, e, (uint32_t)(8 - k), &up);
    }
    D = (uint32_t)ip + (up ? 1u : 0u);
    if (D == 1000000000u) {
      D = 100000000u;
      ++k;
    }
  }
  // the nine digits as characters, the first in the lowest byte; nd = the digits that stay once the trailing zeros are gone
  uint64_t s_lo = 0, s_hi = 0;
  uint32_t nd = 0, x = D;
#pragma unroll
  for (int i = 8; i >= 0; --i) {
    const uint32_t y = x / 10, d = x - y * 10;
    x = y;
    if (nd == 0 && d) nd = (uint32_t)i + 1;
    if (i == 8) s_hi = '0' + d; else s_lo |= (uint64_t)('0' + d) << (8 * i);
  }
  const u128 S = (u128)s_hi << 64 | s_lo;
  u128 line = 0;
  uint32_t len = 0;
#define DFH_PT_PUT(w, n) do { line |= (u128)(w) << (8 * len); len += (n); } while (0)
  if (neg) DFH_PT_PUT('-', 1);
  if (k < -4 || k >= 9) {
    DFH_PT_PUT(S & 0xFF, 1);
    if (nd > 1) {
      DFH_PT_PUT('.', 1);
      DFH_PT_PUT((S >> 8) & pt_mask(nd - 1), nd - 1);
    }
    const uint32_t ak = (uint32_t)(k < 0 ? -k : k);
    DFH_PT_PUT((uint32_t)'e' | (uint32_t)(k < 0 ? '-' : '+') << 8 | ('0' + ak / 10) << 16 | ('0' + ak % 10) << 24, 4);
  } else if (k >= 0) {
    const uint32_t ni = (uint32_t)k + 1;   // digits in front of the point
    DFH_PT_PUT(S & pt_mask(ni), ni);
    if (nd > ni) {
      DFH_PT_PUT('.', 1);
      DFH_PT_PUT((S >> (8 * ni)) & pt_mask(nd - ni), nd - ni);
    }
  } else {
    const uint32_t z = (uint32_t)(-k - 1);   // zeros behind the point: 0 .. 3
    DFH_PT_PUT('0' | '.' << 8, 2);
    if (z) DFH_PT_PUT(0x303030u & (uint32_t)pt_mask(z), z);
    DFH_PT_PUT(S & pt_mask(nd), nd);
  }
  DFH_PT_PUT('\n', 1);
#undef DFH_PT_PUT
  L.lo = (uint64_t)line;
  L.hi = (uint64_t)(line >> 64);
  L.len = len;
  return L;
}

}  // namespace dfh_pt
#endif  // DFH_PREDTEXT_FMT_H_
