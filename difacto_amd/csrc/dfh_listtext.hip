// dfh_listtext.hip — the lines of explain_out and recommend_out on the device (included behind dfh_recommend.hip; pred_write =
// device of task = predict): the lists a dfh_explain or a dfh_recommend holds, read IN PLACE, as the bytes the learner's
// snprintf loops write — "<inter>" and "\t<id_i>:<id_j>:<c>" per pair, or "<item>:<logit>" joined by tabs, and a '\n'.  Ragged
// lines of lists: a head field and 0 .. 32 entries of two or three tokens each, where a dump line has one field per lane and a
// count V_dim fixes.  The arithmetic is dfh_listtext_fmt.h over dfh_predtext_fmt.h and dfh_dumptext_fmt.h; a float pt_format
// does not format is counted, and the caller formats such a unit on the host from dfh_explain_read / dfh_recommend_read.
// dfh_explain_format / dfh_recommend_format are the two passes of dfh_textout.hip with k_listtext<KIND, *>, the rows' lengths
// carried between them, and the object's non-finite count read back in the same round trip: a tile is T = min(1024, floor(32768 /
// the longest line of K)) rows.  A row is P = the power of two >= K + 1 lanes (P <= 64): lane 0 the head (inter; nothing for
// recommend), lane e + 1 entry e, so a wave holds 64 / P rows per round and a row is ONE round.  A lane computes its entry's
// length from its ids (or its item) and its float, a lane past n[r] contributes 0, an inclusive scan inside the P lanes gives
// each entry its offset in the line.  Like k_predtext and k_dumptext these kernels are not in the timing registry
// (dfh_kernel_name) and no other launch changes.
#include "dfh_listtext_fmt.h"

namespace {
enum { LT_EXPLAIN = 0, LT_RECOMMEND = 1 };

// the unit's lists, row r's entries at [r * K ..]
struct LtSrc {
  const uint32_t* n;       // [count]
  const uint32_t* head;    // [count] the bits of inter (explain)
  const uint64_t *ids_i, *ids_j;   // [count * K] (explain)
  const uint32_t* item;    // [count * K] (recommend)
  const uint32_t* val;     // [count * K] the bits of c / of the logit
};

inline uint32_t lt_tile(int kind, uint32_t K) {
  const uint64_t line = kind == LT_EXPLAIN ? dfh_lt::lt_explain_max_line(K) : dfh_lt::lt_recommend_max_line(K);
  return (uint32_t)std::min<uint64_t>(TO_TILE_MAX, TO_IMG / line);   // K <= 32: at least 17
}

// EMIT = 0: rlen[r], tile_bytes[t] (and tile_bytes[ntiles] = 0), *irregular.  EMIT = 1: rlen and tile_scan in, text out.
template <int KIND, int EMIT>
__global__ void __launch_bounds__(256) k_listtext(LtSrc src, uint64_t count, uint32_t K, uint32_t T, uint32_t lp, uint32_t* __restrict__ rlen,
                                                  uint64_t* __restrict__ tile_bytes, const uint64_t* __restrict__ tile_scan,
                                                  unsigned char* __restrict__ out, uint32_t* __restrict__ irregular) {
  __shared__ uint32_t s_acc[2];                          // EMIT = 0: the tile's bytes, its irregular floats
  __shared__ typename TextScan::storage_type s_scan;     // EMIT = 1
  __shared__ uint32_t s_off[EMIT ? TO_TILE_MAX : 1];     // EMIT = 1: where each row's line starts in the tile's text
  __shared__ __attribute__((aligned(16))) unsigned char img[EMIT ? TO_IMG + 16 : 16];
  const uint32_t P = 1u << lp, G = 64u >> lp;         // lanes per row; rows per wave and round
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, g = lane & (P - 1u), lead = lane & ~(P - 1u);
  const uint64_t base = (uint64_t)blockIdx.x * T;
  const uint32_t tn = (uint32_t)(count - base < (uint64_t)T ? count - base : (uint64_t)T);   // rows of this tile: 1 .. T
  TextTile tt = {};
  if (!EMIT)
    to_measure_begin(s_acc);
  else
    tt = to_tile_begin(rlen, base, tn, tile_scan, s_off, s_scan);
  uint32_t irr = 0;
  for (uint32_t r0 = wave * G; r0 < tn; r0 += 4 * G) {   // the same trips for every lane of a wave
    const uint32_t lr = r0 + (lane >> lp);
    const bool valid = lr < tn;
    const uint64_t row = base + (valid ? lr : 0u);
    const uint32_t nr = valid ? min(src.n[row], K) : 0u;   // a list never has more than K entries: a line never leaves its room
    const bool entry = g >= 1u && g - 1u < nr;
    const size_t at_e = (size_t)row * K + (g - 1u);
    dfh_pt::Line H;
    H.lo = H.hi = 0;
    H.len = 0;
    dfh_lt::ExEntry X;
    dfh_lt::RcEntry Y;
    uint32_t len = 0;
    if (KIND == LT_EXPLAIN) {
      if (valid && g == 0) {
        H = dfh_lt::lt_head(src.head[row]);
        len = H.len;
        irr += H.len == 0 ? 1u : 0u;
      }
      if (entry) {
        X = dfh_lt::lt_explain_entry(src.ids_i[at_e], src.ids_j[at_e], src.val[at_e]);
        len = X.len;
        irr += X.v.len == 0 ? 1u : 0u;
      }
    } else if (entry) {
      Y = dfh_lt::lt_recommend_entry(src.item[at_e], src.val[at_e], g == 1u);
      len = Y.len;
      irr += Y.v.len == 0 ? 1u : 0u;
    }
    uint32_t total;   // the line without its '\n'
    const uint32_t x = to_group_scan(len, P, g, lead, &total);
    if (!EMIT) {
      if (valid && g == 0) {
        rlen[row] = total + 1;
        atomicAdd(&s_acc[0], total + 1);
      }
    } else {
      unsigned char* const p = img + tt.run0 + s_off[valid ? lr : 0] + (x - len);   // at most 15 + T * the longest line <= 15 + TO_IMG behind img
      if (KIND == LT_EXPLAIN) {
        if (valid && g == 0) dfh_pt::pt_put(p, H.lo, H.hi, H.len);
        if (entry) dfh_lt::lt_put_explain_entry(p, X);
      } else if (entry) {
        dfh_lt::lt_put_recommend_entry(p, Y);
      }
      if (valid && g == 0) p[total] = '\n';   // lane 0's place is the line's first byte
    }
  }
  if (!EMIT) {
    to_measure_end(s_acc, irr, tile_bytes, irregular);
    return;
  }
  __syncthreads();   // the image is complete
  to_store(out, img, tt.g_first, tt.g_end, tt.g_img);
}

// Formats rows [0, count) of src; one wait.  The caller has cleared its `formatted` and sets it on DFH_OK.
template <int KIND>
int lt_format(dfh_ctx* c, TextWork* w, const LtSrc& src, size_t count, uint32_t K, const unsigned long long* d_nf, const char* who,
              size_t* nbytes, uint64_t* irregular) {
  hipStream_t s = c->stream;
  const uint32_t T = lt_tile(KIND, K);
  uint32_t lp = 0;
  while ((1u << lp) < K + 1u) ++lp;   // K <= 32: P <= 64
  const uint64_t max_line = KIND == LT_EXPLAIN ? dfh_lt::lt_explain_max_line(K) : dfh_lt::lt_recommend_max_line(K);
  return to_format(c, w, count, T, (size_t)max_line, true, d_nf, who,
                   [&](int emit, unsigned ntiles, const TextPass& a) {
                     hipLaunchKernelGGL((emit ? k_listtext<KIND, 1> : k_listtext<KIND, 0>), dim3(ntiles), dim3(256), 0, s, src, (uint64_t)count,
                                        K, T, lp, a.rlen, a.tile_bytes, a.tile_scan, a.out, a.irregular);
                   },
                   nbytes, irregular);
}

int lt_nonfinite(const TextWork* w, bool formatted, uint64_t* nonfinite, const char* who) {
  DFH_ARG(nonfinite, std::string(who) + ": NULL argument");
  *nonfinite = 0;
  if (!formatted) {
    set_error(std::string(who) + ": nothing formatted (the count is the one the last format read back)");
    return DFH_ERR_STATE;
  }
  *nonfinite = w->nonfinite;
  return DFH_OK;
}
}  // namespace

extern "C" {

int dfh_explain_format(dfh_explain* e, size_t* nbytes, uint64_t* irregular) {
  DFH_ARG(e && nbytes && irregular, "dfh_explain_format: NULL argument");
  *nbytes = 0;
  *irregular = 0;
  DFH_HIP(hipSetDevice(e->ctx->device));
  e->formatted = false;
  LtSrc src = {};
  if (e->n) {
    const ExOut o = ex_arrays(e->d_out, e->cap, e->K, 0);
    src.n = o.n;
    src.head = reinterpret_cast<const uint32_t*>(o.inter);
    src.ids_i = o.ids_i;
    src.ids_j = o.ids_j;
    src.val = reinterpret_cast<const uint32_t*>(o.c);
  }
  const int rc = lt_format<LT_EXPLAIN>(e->ctx, &e->text, src, e->n, e->K, e->d_nf, "dfh_explain_format", nbytes, irregular);
  if (rc) return rc;
  ex_free_retired(e);
  e->formatted = true;
  return DFH_OK;
}

int dfh_explain_read_text(dfh_explain* e, char* dst) {
  DFH_ARG(e, "dfh_explain_read_text: NULL argument");
  if (!e->formatted) {
    set_error("dfh_explain_read_text: nothing formatted (call the object's format after the last append or reset)");
    return DFH_ERR_STATE;
  }
  DFH_ARG(dst || e->text.text_bytes == 0, "dfh_explain_read_text: NULL argument");
  return to_read(e->ctx, &e->text, dst);
}

int dfh_explain_text_nonfinite(dfh_explain* e, uint64_t* nonfinite) {
  DFH_ARG(e, "dfh_explain_text_nonfinite: NULL argument");
  return lt_nonfinite(&e->text, e->formatted, nonfinite, "dfh_explain_text_nonfinite");
}

int dfh_explain_text_tile(dfh_explain* e) { return e ? (int)lt_tile(LT_EXPLAIN, e->K) : 0; }

int dfh_recommend_format(dfh_recommend* r, size_t* nbytes, uint64_t* irregular) {
  DFH_ARG(r && nbytes && irregular, "dfh_recommend_format: NULL argument");
  *nbytes = 0;
  *irregular = 0;
  DFH_HIP(hipSetDevice(r->ctx->device));
  r->formatted = false;
  LtSrc src = {};
  if (r->n) {
    const RcOut o = rc_arrays(r->d_out, r->cap, r->K, 0);
    src.n = o.n;
    src.item = o.item;
    src.val = reinterpret_cast<const uint32_t*>(o.logit);
  }
  const int rc = lt_format<LT_RECOMMEND>(r->ctx, &r->text, src, r->n, r->K, r->d_nf, "dfh_recommend_format", nbytes, irregular);
  if (rc) return rc;
  rc_free_retired(r);
  r->formatted = true;
  return DFH_OK;
}

int dfh_recommend_read_text(dfh_recommend* r, char* dst) {
  DFH_ARG(r, "dfh_recommend_read_text: NULL argument");
  if (!r->formatted) {
    set_error("dfh_recommend_read_text: nothing formatted (call the object's format after the last append or reset)");
    return DFH_ERR_STATE;
  }
  DFH_ARG(dst || r->text.text_bytes == 0, "dfh_recommend_read_text: NULL argument");
  return to_read(r->ctx, &r->text, dst);
}

int dfh_recommend_text_nonfinite(dfh_recommend* r, uint64_t* nonfinite) {
  DFH_ARG(r, "dfh_recommend_text_nonfinite: NULL argument");
  return lt_nonfinite(&r->text, r->formatted, nonfinite, "dfh_recommend_text_nonfinite");
}

int dfh_recommend_text_tile(dfh_recommend* r) { return r ? (int)lt_tile(LT_RECOMMEND, r->K) : 0; }

}  // extern "C"
