// dfh_listtext.hip — the lines of explain_out and recommend_out on the device (included behind dfh_recommend.hip; pred_write =
// device of task = predict): the lists a dfh_explain or a dfh_recommend holds, read IN PLACE, as the bytes the learner's
// snprintf loops write — "<inter>" and "\t<id_i>:<id_j>:<c>" per pair, or "<item>:<logit>" joined by tabs, and a '\n'.  Ragged
// lines of lists: a head field and 0 .. 32 entries of two or three tokens each, where a dump line has one field per lane and a
// count V_dim fixes.  The arithmetic is dfh_listtext_fmt.h over dfh_predtext_fmt.h and dfh_dumptext_fmt.h; a float pt_format
// does not format is counted, and the caller formats such a unit on the host from dfh_explain_read / dfh_recommend_read.
// dfh_explain_format / dfh_recommend_format queue, in the shape of k_dumptext:
//   k_listtext<KIND, 0>  a block per tile of T rows, T = min(1024, floor(32768 / the longest line of K)).  A row is P = the power
//                        of two >= K + 1 lanes (P <= 64): lane 0 the head (inter; nothing for recommend), lane e + 1 entry e, so
//                        a wave holds 64 / P rows per round and a row is ONE round.  A lane computes its entry's length from its
//                        ids (or its item) and its float, a lane past n[r] contributes 0, an inclusive scan inside the P lanes
//                        gives each entry its offset in the line.  Out: each row's length (4 B), the tile's bytes, the irregular
//                        floats (an atomic per block that has any)
//   rocprim::exclusive_scan over the tiles' bytes
//   k_listtext<KIND, 1>  a block per tile again: the rows' lengths scanned in the block place the lines in an LDS image of 32 KB,
//                        each lane formats its entry ONCE MORE straight into its place (4 B per row is all the passes share), the
//                        image is shifted by the tile's first byte mod 16 and written with aligned 16 B stores; only the tile's
//                        unaligned head and tail go byte by byte
// and read back {bytes, irregular, the object's non-finite count}: one host round trip.  The launches are ordered by the stream
// alone: no block waits for another.  Plain C++, vector stores, no scratch.  Like k_predtext and k_dumptext these kernels are
// not in the timing registry (dfh_kernel_name) and no other launch changes.
#include "dfh_listtext_fmt.h"

// a format's workspace, grown to what a format needs, kept with its object
struct LtWork {
  char* d_text = nullptr;
  size_t text_cap = 0, text_bytes = 0;
  uint32_t* d_rlen = nullptr;     // [rlen_cap] bytes per row of the unit
  size_t rlen_cap = 0;
  uint64_t *d_tile = nullptr, *d_tile_scan = nullptr;   // bytes per tile (and a 0), their exclusive scan (the last: all bytes)
  size_t tile_cap = 0, scan_cap = 0;
  void* d_tmp = nullptr;          // rocprim's
  size_t tmp_bytes = 0;
  uint32_t* d_irr = nullptr;      // the irregular floats of the last format
  uint64_t* h_head = nullptr;     // page-locked {bytes, irregular, non-finite}
  char* h_text = nullptr;         // page-locked: read_text's download lands here
  size_t h_text_cap = 0;
  uint64_t nonfinite = 0;         // of the last format
};

namespace {
constexpr uint32_t LT_IMG = 32768, LT_TILE_MAX = 1024;   // the LDS image of a tile's text (and 16 B for its shift); rows per tile at most
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
  return (uint32_t)std::min<uint64_t>(LT_TILE_MAX, LT_IMG / line);   // K <= 32: at least 17
}

// EMIT = 0: rlen[r], tile_bytes[t] (and tile_bytes[ntiles] = 0), *irregular.  EMIT = 1: rlen and tile_scan in, text out.
template <int KIND, int EMIT>
__global__ void __launch_bounds__(256) k_listtext(LtSrc src, uint64_t count, uint32_t K, uint32_t T, uint32_t lp, uint32_t* __restrict__ rlen,
                                                  uint64_t* __restrict__ tile_bytes, const uint64_t* __restrict__ tile_scan,
                                                  unsigned char* __restrict__ out, uint32_t* __restrict__ irregular) {
  using Scan = rocprim::block_scan<uint32_t, 256>;
  __shared__ uint32_t s_acc[2];                       // EMIT = 0: the tile's bytes, its irregular floats
  __shared__ typename Scan::storage_type s_scan;      // EMIT = 1
  __shared__ uint32_t s_off[EMIT ? LT_TILE_MAX : 1];  // EMIT = 1: where each row's line starts in the tile's text
  __shared__ __attribute__((aligned(16))) unsigned char img[EMIT ? LT_IMG + 16 : 16];
  const uint32_t P = 1u << lp, G = 64u >> lp;         // lanes per row; rows per wave and round
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, g = lane & (P - 1u), lead = lane & ~(P - 1u);
  const uint64_t base = (uint64_t)blockIdx.x * T;
  const uint32_t tn = (uint32_t)(count - base < (uint64_t)T ? count - base : (uint64_t)T);   // rows of this tile: 1 .. T
  uint64_t g_first = 0, g_end = 0, g_img = 0;
  uint32_t run0 = 0;
  if (!EMIT) {
    if (threadIdx.x < 2) s_acc[threadIdx.x] = 0;
    __syncthreads();
  } else {
    uint32_t len4[4], off4[4];
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) {
      const uint32_t r = 4 * threadIdx.x + i;
      len4[i] = r < tn ? rlen[base + r] : 0u;
    }
    Scan().exclusive_scan(len4, off4, 0u, s_scan);
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) s_off[4 * threadIdx.x + i] = off4[i];   // 4 * 256 = LT_TILE_MAX
    g_first = tile_scan[blockIdx.x];
    g_end = tile_scan[blockIdx.x + 1];
    g_img = g_first & ~15ULL;   // the text position of img[0]: a 16 B word of the text is a 16 B word of the image
    run0 = (uint32_t)(g_first - g_img);
    __syncthreads();
  }
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
    uint32_t x = len;   // inclusive scan inside the row's P lanes
    for (uint32_t o = 1; o < P; o <<= 1) {
      const uint32_t y = (uint32_t)__shfl_up((int)x, o, 64);
      if (g >= o) x += y;
    }
    const uint32_t total = (uint32_t)__shfl((int)x, (int)(lead + P - 1u), 64);   // the line without its '\n'
    if (!EMIT) {
      if (valid && g == 0) {
        rlen[row] = total + 1;
        atomicAdd(&s_acc[0], total + 1);
      }
    } else {
      unsigned char* const p = img + run0 + s_off[valid ? lr : 0] + (x - len);   // at most 15 + T * the longest line <= 15 + LT_IMG behind img
      if (KIND == LT_EXPLAIN) {
        if (valid && g == 0) dfh_lt::lt_put_bytes(p, H.lo, H.hi, H.len);
        if (entry) dfh_lt::lt_put_explain_entry(p, X);
      } else if (entry) {
        dfh_lt::lt_put_recommend_entry(p, Y);
      }
      if (valid && g == 0) p[total] = '\n';   // lane 0's place is the line's first byte
    }
  }
  if (!EMIT) {
    if (irr) atomicAdd(&s_acc[1], irr);
    __syncthreads();
    if (threadIdx.x == 0) {
      tile_bytes[blockIdx.x] = s_acc[0];
      if (blockIdx.x == 0) tile_bytes[gridDim.x] = 0;
      if (s_acc[1]) atomicAdd(irregular, s_acc[1]);
    }
    return;
  }
  __syncthreads();   // the image is complete
  const uint64_t a0 = (g_first + 15) & ~15ULL, a1 = g_end & ~15ULL;   // the aligned words lie in [a0, a1)
  const uint64_t head_end = a0 < g_end ? a0 : g_end;
  for (uint64_t q = g_first + threadIdx.x; q < head_end; q += 256) out[q] = img[q - g_img];
  for (uint64_t q = a0 + 16ULL * threadIdx.x; q < a1; q += 16ULL * 256)
    *reinterpret_cast<uint4*>(out + q) = *reinterpret_cast<const uint4*>(img + (q - g_img));
  for (uint64_t q = (a1 > head_end ? a1 : head_end) + threadIdx.x; q < g_end; q += 256) out[q] = img[q - g_img];
}

void lt_release(LtWork* w) {
  if (!w) return;
  if (w->d_text) (void)hipFree(w->d_text);
  if (w->d_rlen) (void)hipFree(w->d_rlen);
  if (w->d_tile) (void)hipFree(w->d_tile);
  if (w->d_tile_scan) (void)hipFree(w->d_tile_scan);
  if (w->d_tmp) (void)hipFree(w->d_tmp);
  if (w->d_irr) (void)hipFree(w->d_irr);
  if (w->h_head) (void)hipHostFree(w->h_head);
  if (w->h_text) (void)hipHostFree(w->h_text);
  delete w;
}

// the object's workspace, made by its first format
int lt_work(LtWork** wp, const char* who) {
  if (*wp) return DFH_OK;
  LtWork* w = new (std::nothrow) LtWork();
  if (!w) {
    set_error(std::string(who) + ": out of host memory (" + std::to_string(sizeof(LtWork)) + " bytes needed)");
    return DFH_ERR_CAPACITY;
  }
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&w->d_irr), sizeof(uint32_t));
  if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void**>(&w->h_head), 3 * sizeof(uint64_t), hipHostMallocDefault);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    set_error(std::string(who) + ": " + hipGetErrorString(e));
    lt_release(w);
    return DFH_ERR_HIP;
  }
  *wp = w;
  return DFH_OK;
}

// Formats rows [0, count) of src; one wait.  The caller has cleared its `formatted` and sets it on DFH_OK.
template <int KIND>
int lt_format(dfh_ctx* c, LtWork** wp, const LtSrc& src, size_t count, uint32_t K, const unsigned long long* d_nf, const char* who,
              size_t* nbytes, uint64_t* irregular) {
  hipStream_t s = c->stream;
  int rc = lt_work(wp, who);
  if (rc) return rc;
  LtWork* w = *wp;
  w->text_bytes = 0;
  w->nonfinite = 0;
  w->h_head[0] = w->h_head[1] = w->h_head[2] = 0;
  if (count) {
    const uint32_t T = lt_tile(KIND, K);
    uint32_t lp = 0;
    while ((1u << lp) < K + 1u) ++lp;   // K <= 32: P <= 64
    const size_t ntiles = (count + T - 1) / T;
    const uint64_t max_line = KIND == LT_EXPLAIN ? dfh_lt::lt_explain_max_line(K) : dfh_lt::lt_recommend_max_line(K);
    size_t need = 0;
    DFH_HIP(rocprim::exclusive_scan(nullptr, need, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t)0, ntiles + 1, rocprim::plus<uint64_t>(), s));
    rc = dt_grow(&w->d_text, &w->text_cap, count * (size_t)max_line, who, "the text");
    if (!rc) rc = dt_grow(&w->d_rlen, &w->rlen_cap, count, who, "the rows' byte counts");
    if (!rc) rc = dt_grow(&w->d_tile, &w->tile_cap, ntiles + 1, who, "the tiles' byte counts");
    if (!rc) rc = dt_grow(&w->d_tile_scan, &w->scan_cap, ntiles + 1, who, "the tiles' offsets");
    if (!rc) {
      char* tmp = static_cast<char*>(w->d_tmp);
      rc = dt_grow(&tmp, &w->tmp_bytes, std::max<size_t>(need, 256), who, "the scan");
      w->d_tmp = tmp;
    }
    if (rc) return rc;
    DFH_HIP(hipMemsetAsync(w->d_irr, 0, sizeof(uint32_t), s));
    hipLaunchKernelGGL((k_listtext<KIND, 0>), dim3((unsigned)ntiles), dim3(256), 0, s, src, (uint64_t)count, K, T, lp, w->d_rlen, w->d_tile,
                       (const uint64_t*)nullptr, (unsigned char*)nullptr, w->d_irr);
    DFH_HIP(hipGetLastError());
    size_t tb = w->tmp_bytes;
    DFH_HIP(rocprim::exclusive_scan(w->d_tmp, tb, w->d_tile, w->d_tile_scan, (uint64_t)0, ntiles + 1, rocprim::plus<uint64_t>(), s));
    hipLaunchKernelGGL((k_listtext<KIND, 1>), dim3((unsigned)ntiles), dim3(256), 0, s, src, (uint64_t)count, K, T, lp, w->d_rlen, (uint64_t*)nullptr,
                       (const uint64_t*)w->d_tile_scan, reinterpret_cast<unsigned char*>(w->d_text), (uint32_t*)nullptr);
    DFH_HIP(hipGetLastError());
    DFH_HIP(hipMemcpyAsync(&w->h_head[0], w->d_tile_scan + ntiles, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    DFH_HIP(hipMemcpyAsync(&w->h_head[1], w->d_irr, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  }
  DFH_HIP(hipMemcpyAsync(&w->h_head[2], d_nf, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  DFH_HIP(hipStreamSynchronize(s));
  w->text_bytes = (size_t)w->h_head[0];
  w->nonfinite = w->h_head[2];
  *nbytes = w->text_bytes;
  *irregular = w->h_head[1];
  return DFH_OK;
}

// the text of the last format into dst, through page-locked memory of the object's
int lt_read(dfh_ctx* c, LtWork* w, bool formatted, char* dst, const char* who) {
  if (!w || !formatted) {
    set_error(std::string(who) + ": nothing formatted (call the object's format after the last append or reset)");
    return DFH_ERR_STATE;
  }
  const size_t nb = w->text_bytes;
  if (nb == 0) return DFH_OK;
  DFH_ARG(dst, std::string(who) + ": NULL argument");
  DFH_HIP(hipSetDevice(c->device));
  if (nb > w->h_text_cap) {
    if (w->h_text) DFH_HIP(hipHostFree(w->h_text));
    w->h_text = nullptr;
    w->h_text_cap = 0;
    const size_t cap = nb + nb / 4;
    DFH_HIP(hipHostMalloc(reinterpret_cast<void**>(&w->h_text), cap, hipHostMallocDefault));
    w->h_text_cap = cap;
  }
  DFH_HIP(hipMemcpyAsync(w->h_text, w->d_text, nb, hipMemcpyDeviceToHost, c->stream));
  DFH_HIP(hipStreamSynchronize(c->stream));
  memcpy(dst, w->h_text, nb);
  return DFH_OK;
}

int lt_nonfinite(LtWork* w, bool formatted, uint64_t* nonfinite, const char* who) {
  DFH_ARG(nonfinite, std::string(who) + ": NULL argument");
  *nonfinite = 0;
  if (!w || !formatted) {
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
  return lt_read(e->ctx, e->text, e->formatted, dst, "dfh_explain_read_text");
}

int dfh_explain_text_nonfinite(dfh_explain* e, uint64_t* nonfinite) {
  DFH_ARG(e, "dfh_explain_text_nonfinite: NULL argument");
  return lt_nonfinite(e->text, e->formatted, nonfinite, "dfh_explain_text_nonfinite");
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
  return lt_read(r->ctx, r->text, r->formatted, dst, "dfh_recommend_read_text");
}

int dfh_recommend_text_nonfinite(dfh_recommend* r, uint64_t* nonfinite) {
  DFH_ARG(r, "dfh_recommend_text_nonfinite: NULL argument");
  return lt_nonfinite(r->text, r->formatted, nonfinite, "dfh_recommend_text_nonfinite");
}

int dfh_recommend_text_tile(dfh_recommend* r) { return r ? (int)lt_tile(LT_RECOMMEND, r->K) : 0; }

}  // extern "C"
