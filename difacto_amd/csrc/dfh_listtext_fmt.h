// dfh_listtext_fmt.h — a line of explain_out and of recommend_out of task = predict, in integer arithmetic: everything of them
// that is not dfh_pt::pt_format (dfh_predtext_fmt.h) and dfh_dt::dt_id / dt_put_id / dt_field (dfh_dumptext_fmt.h), used as they
// are.  Plain C++ like those headers, so a host program can compile the same functions and compare them with the C library; the
// device formatter (dfh_listtext.hip) calls the entry functions per lane.
//
//   explain_out    "<inter>" then "\t<id_i>:<id_j>:<c>" per pair, then "\n": %.9g, %llu, %llu, %.9g.
//                  head   pt_format's line of inter without its '\n': at most 15 bytes (0: inter is not regular)
//                  entry  '\t', the nd characters of id_i, ':', those of id_j, and dt_field of c with a ':' in the place of its
//                         '\t': at most 1 + 20 + 1 + 20 + 1 + 15 = 58 bytes
//                  line   at most 15 + 58 K + 1 bytes
//   recommend_out  "<item>:<logit>" per entry, joined by '\t', then "\n": %u, %.9g.  No entry: the single byte '\n'.
//                  entry  a '\t' unless it is the first, the item's digits (at most 10), and the ':' field of the logit: at most
//                         1 + 10 + 1 + 15 = 27 bytes
//                  line   at most 27 K + 1 bytes
// An entry whose float is not regular has the length of its other characters and is counted by the caller: the line is then not
// valid, and nothing is written outside the room of a valid one.
#ifndef DFH_LISTTEXT_FMT_H_
#define DFH_LISTTEXT_FMT_H_
#include "dfh_dumptext_fmt.h"

namespace dfh_lt {

constexpr uint32_t LT_MAX_VALUE = dfh_pt::PT_MAX_LINE - 1;   // the characters of %.9g
constexpr uint32_t LT_EX_ENTRY = 1 + dfh_dt::DT_ID_CHARS + 1 + dfh_dt::DT_ID_CHARS + 1 + LT_MAX_VALUE, LT_RC_ITEM_CHARS = 10,
                   LT_RC_ENTRY = 1 + LT_RC_ITEM_CHARS + 1 + LT_MAX_VALUE;
static_assert(LT_EX_ENTRY == 58 && LT_RC_ENTRY == 27, "the entries' bounds follow PT_MAX_LINE");

DFH_PT_FN uint64_t lt_explain_max_line(uint64_t K) { return LT_MAX_VALUE + LT_EX_ENTRY * K + 1; }
DFH_PT_FN uint64_t lt_recommend_max_line(uint64_t K) { return LT_RC_ENTRY * K + 1; }

// ':' and the text of %.9g: dt_field with the ':' where its '\t' is.  len 2 .. 16; 0: the value is not regular
DFH_PT_FN dfh_dt::Field lt_value(uint32_t bits) {
  dfh_dt::Field F = dfh_dt::dt_field(bits);
  F.lo = (F.lo & ~0xFFULL) | (uint64_t)':';
  return F;
}

// the head of an explain line: pt_format's line, its '\n' not counted.  len 1 .. 15; 0: the value is not regular
DFH_PT_FN dfh_pt::Line lt_head(uint32_t bits) {
  dfh_pt::Line L = dfh_pt::pt_format(bits);
  if (L.len) --L.len;
  return L;
}

struct ExEntry {
  dfh_dt::Id a, b;
  dfh_dt::Field v;
  uint32_t len;   // 1 + a.nd + 1 + b.nd + v.len
};

DFH_PT_FN ExEntry lt_explain_entry(uint64_t id_i, uint64_t id_j, uint32_t c_bits) {
  ExEntry E;
  E.a = dfh_dt::dt_id(id_i);
  E.b = dfh_dt::dt_id(id_j);
  E.v = lt_value(c_bits);
  E.len = 2u + E.a.nd + E.b.nd + E.v.len;
  return E;
}

DFH_PT_FN void lt_put_explain_entry(unsigned char* p, const ExEntry& E) {
  p[0] = '\t';
  dfh_dt::dt_put_id(p + 1, E.a);
  p[1 + E.a.nd] = ':';
  dfh_dt::dt_put_id(p + 2 + E.a.nd, E.b);
  dfh_dt::dt_put_field(p + 2 + E.a.nd + E.b.nd, E.v);
}

struct RcEntry {
  uint32_t c_hi;   // the zero-padded 10 characters of the item: two in c_hi, eight in c_lo, the first in the lowest byte
  uint64_t c_lo;
  uint32_t nd, tab;   // 1 .. 10: the characters that count, the LAST nd of the 10; 1: a '\t' in front
  dfh_dt::Field v;
  uint32_t len;       // tab + nd + v.len
};

DFH_PT_FN RcEntry lt_recommend_entry(uint32_t item, uint32_t logit_bits, bool first) {
  RcEntry E;
  const uint32_t top = item / 100000000u, low = item - top * 100000000u;   // top <= 42
  E.c_hi = ('0' + top / 10u) | ('0' + top % 10u) << 8;
  E.c_lo = dfh_dt::dt_chars8(low);
  E.nd = top ? (top >= 10u ? 10u : 9u) : dfh_dt::dt_ndigits8(low);
  E.tab = first ? 0u : 1u;
  E.v = lt_value(logit_bits);
  E.len = E.tab + E.nd + E.v.len;
  return E;
}

DFH_PT_FN void lt_put_recommend_entry(unsigned char* p, const RcEntry& E) {
  if (E.tab) p[0] = '\t';
  unsigned char* const q = p + E.tab;
  const uint32_t skip = LT_RC_ITEM_CHARS - E.nd;
#pragma unroll
  for (uint32_t b = 0; b < 2; ++b)
    if (b >= skip) q[b - skip] = (unsigned char)(E.c_hi >> (8 * b));
#pragma unroll
  for (uint32_t b = 0; b < 8; ++b)
    if (2 + b >= skip) q[2 + b - skip] = (unsigned char)(E.c_lo >> (8 * b));
  dfh_dt::dt_put_field(q + E.nd, E.v);
}

// One whole line into dst (room for lt_*_max_line(K) bytes with n <= K), serially: what the device lays out with a scan over the
// lanes of a row.  Returns the line's length; *irregular grows by the floats that were not formatted (the line is then not valid).
DFH_PT_FN uint32_t lt_explain_line(unsigned char* dst, uint32_t inter_bits, uint32_t n, const uint64_t* ids_i, const uint64_t* ids_j,
                                   const uint32_t* c_bits, uint32_t* irregular) {
  const dfh_pt::Line H = lt_head(inter_bits);
  if (H.len == 0) ++*irregular;
  dfh_pt::pt_put(dst, H.lo, H.hi, H.len);
  uint32_t at = H.len;
  for (uint32_t j = 0; j < n; ++j) {
    const ExEntry E = lt_explain_entry(ids_i[j], ids_j[j], c_bits[j]);
    if (E.v.len == 0) ++*irregular;
    lt_put_explain_entry(dst + at, E);
    at += E.len;
  }
  dst[at] = '\n';
  return at + 1;
}

DFH_PT_FN uint32_t lt_recommend_line(unsigned char* dst, uint32_t n, const uint32_t* items, const uint32_t* logit_bits, uint32_t* irregular) {
  uint32_t at = 0;
  for (uint32_t j = 0; j < n; ++j) {
    const RcEntry E = lt_recommend_entry(items[j], logit_bits[j], j == 0);
    if (E.v.len == 0) ++*irregular;
    lt_put_recommend_entry(dst + at, E);
    at += E.len;
  }
  dst[at] = '\n';
  return at + 1;
}

}  // namespace dfh_lt
#endif  // DFH_LISTTEXT_FMT_H_
