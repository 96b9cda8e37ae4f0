// dfh_dumptext_fmt.h — a line of task = dump, "<id>\t<w>[\t<V_0> .. \t<V_{k-1}>]\n", in integer arithmetic: everything of it
// that is not dfh_pt::pt_format (dfh_predtext_fmt.h, used as it is).  Plain C++ like that header, so a host program can compile
// the same functions and compare them with the C library; the device formatter (dfh_dumptext.hip) calls them per lane.
//
//   <id>    %llu of an unsigned 64-bit id: the 20 characters of the zero-padded decimal form and how many of them count
//           (dt_id: three constant divisions split the id into 4 + 8 + 8 digits, which are 32-bit work; dt_put_id writes the
//           nd characters that count)
//   field   '\t' and the text of %.9g: pt_format's line moved up one byte, a '\t' in its first byte, its '\n' falling off the
//           end — a field has exactly as many bytes as pt_format's line, at most 16; 0: the value is not regular (not
//           formatted, counted by the caller)
//   line    the id's nd characters at 0, field j at nd + the lengths of the fields before it, '\n' behind the last field.
//           An entry without V has the one field of w, whatever V_dim is.  The longest line: 20 + 16 (1 + V_dim) + 1 bytes.
#ifndef DFH_DUMPTEXT_FMT_H_
#define DFH_DUMPTEXT_FMT_H_
#include "dfh_predtext_fmt.h"

namespace dfh_dt {

constexpr uint32_t DT_ID_CHARS = 20, DT_MAX_FIELD = dfh_pt::PT_MAX_LINE;

DFH_PT_FN uint64_t dt_max_line(uint64_t V_dim) { return DT_ID_CHARS + DT_MAX_FIELD * (1 + V_dim) + 1; }

// the zero-padded 20 characters of an id, text byte b in: c0 >> 8 b (b < 4), c1 >> 8 (b - 4) (b < 12), c2 >> 8 (b - 12)
struct Id {
  uint32_t c0;
  uint64_t c1, c2;
  uint32_t nd;   // 1 .. 20: the characters that count, the LAST nd of the 20
};

// the eight characters of x < 10^8, the first digit in the lowest byte
DFH_PT_FN uint64_t dt_chars8(uint32_t x) {
  uint64_t s = 0;
#pragma unroll
  for (int i = 7; i >= 0; --i) {
    const uint32_t y = x / 10, d = x - y * 10;
    x = y;
    s |= (uint64_t)('0' + d) << (8 * i);
  }
  return s;
}

// decimal digits of x < 10^8 (1 for x = 0)
DFH_PT_FN uint32_t dt_ndigits8(uint32_t x) {
  return 1u + (x >= 10u) + (x >= 100u) + (x >= 1000u) + (x >= 10000u) + (x >= 100000u) + (x >= 1000000u) + (x >= 10000000u);
}

DFH_PT_FN Id dt_id(uint64_t id) {
  const uint64_t top = id / 10000000000000000ULL, rest = id - top * 10000000000000000ULL;   // top <= 1844
  const uint32_t mid = (uint32_t)(rest / 100000000ULL), low = (uint32_t)(rest - (uint64_t)mid * 100000000ULL);
  Id d;
  d.c0 = (uint32_t)(dt_chars8((uint32_t)top) >> 32);
  d.c1 = dt_chars8(mid);
  d.c2 = dt_chars8(low);
  d.nd = top ? 16u + dt_ndigits8((uint32_t)top) : (mid ? 8u + dt_ndigits8(mid) : dt_ndigits8(low));
  return d;
}

// the id's nd characters to p[0 .. nd)
DFH_PT_FN void dt_put_id(unsigned char* p, const Id& d) {
  const uint32_t skip = DT_ID_CHARS - d.nd;
#pragma unroll
  for (uint32_t b = 0; b < 4; ++b)
    if (b >= skip) p[b - skip] = (unsigned char)(d.c0 >> (8 * b));
#pragma unroll
  for (uint32_t b = 0; b < 8; ++b)
    if (4 + b >= skip) p[4 + b - skip] = (unsigned char)(d.c1 >> (8 * b));
#pragma unroll
  for (uint32_t b = 0; b < 8; ++b)
    if (12 + b >= skip) p[12 + b - skip] = (unsigned char)(d.c2 >> (8 * b));
}

struct Field {
  uint64_t lo, hi;   // the bytes of the field, the '\t' in the lowest byte of lo
  uint32_t len;      // 2 .. 16; 0: the value is not regular
};

DFH_PT_FN Field dt_field(uint32_t bits) {
  const dfh_pt::Line L = dfh_pt::pt_format(bits);
  Field F;
  F.hi = L.hi << 8 | L.lo >> 56;
  F.lo = L.lo << 8 | (uint64_t)'\t';
  F.len = L.len;   // the '\n' sits at byte len now: outside the field
  return F;
}

DFH_PT_FN void dt_put_field(unsigned char* p, const Field& F) {
#pragma unroll
  for (uint32_t b = 0; b < 8; ++b)
    if (b < F.len) p[b] = (unsigned char)(F.lo >> (8 * b));
#pragma unroll
  for (uint32_t b = 0; b < 8; ++b)
    if (8 + b < F.len) p[8 + b] = (unsigned char)(F.hi >> (8 * b));
}

// One whole line into dst (room for dt_max_line(V_dim) bytes), serially: what the device lays out with a scan over the lanes
// of an entry.  Returns the line's length; *irregular grows by the values that were not formatted (the line is then not valid:
// their fields are missing).  V_bits [V_dim] is read only when has_V.
DFH_PT_FN uint32_t dt_line(unsigned char* dst, uint64_t id, uint32_t w_bits, bool has_V, const uint32_t* V_bits, uint32_t V_dim,
                           uint32_t* irregular) {
  const Id d = dt_id(id);
  dt_put_id(dst, d);
  uint32_t at = d.nd;
  const uint32_t nv = 1 + (has_V ? V_dim : 0u);
  for (uint32_t j = 0; j < nv; ++j) {
    const Field F = dt_field(j == 0 ? w_bits : V_bits[j - 1]);
    if (F.len == 0) ++*irregular;
    dt_put_field(dst + at, F);
    at += F.len;
  }
  dst[at] = '\n';
  return at + 1;
}

}  // namespace dfh_dt
#endif  // DFH_DUMPTEXT_FMT_H_
