// dfh_predtext.hip — prediction text on the device: the bytes fprintf("%.9g\n", v) writes for every prediction appended since
// the last reset, concatenated in order (included at the end of dfh_api.hip; the learner's pred_write = device).  Modelled on
// dfh_eval.hip for everything but the arithmetic: the appended values sit in one device array that grows by doubling, appends
// are copies queued on the context's stream, a replaced array is freed behind the next wait.
// The arithmetic is dfh_predtext_fmt.h: exact, integer only, for the REGULAR values (+-0 and 2^-64 <= |v| < 2^32).  Anything
// else is counted, and the caller formats such a set on the host — the idiom of the parse and decode kernels.
// dfh_predtext_format queues
//   k_predtext<0>   a block per tile of PT_TILE values, a lane per value and round: the line's length; the tile's bytes, and the
//                   irregular values of the tile added to the one counter the blocks share (an atomic per block that has any)
//   rocprim::exclusive_scan over the tiles' bytes
//   k_predtext<1>   a block per tile again: the lines are formatted ONCE MORE (nothing but 4 B per value is carried between the
//                   passes: a 16 B slot per value would cost 33 B of traffic per value to save ~250 integer instructions) and
//                   laid out in LDS at their scanned offsets, the image shifted by the tile's first byte mod 16; then the block
//                   writes the image with aligned 16 B stores, and only the tile's unaligned head and tail byte by byte (two
//                   neighbouring tiles meet inside one 16 B word: each writes its own bytes of it)
// and reads back {bytes, irregular} — one host round trip.  The launches are ordered by the stream alone: no block waits for
// another.  Plain C++, no scratch.  These kernels are not in the timing registry (dfh_kernel_name) and no launch of a step
// changes.
#include "dfh_predtext_fmt.h"

struct dfh_predtext {
  dfh_ctx* ctx = nullptr;
  float* d_val = nullptr;       // [cap] the appended values
  size_t cap = 0, n = 0, hint = 0;
  std::vector<void*> retired;   // arrays a growth replaced: copies out of them may still be queued, freed behind the next wait
  // format's workspace, grown to what a format needs, kept
  char* d_text = nullptr;       // [text_cap] the text of the last format
  size_t text_cap = 0, text_bytes = 0;
  uint64_t *d_tile = nullptr, *d_tile_scan = nullptr;   // [tile_cap] bytes per tile (and a 0), their exclusive scan (the last: all bytes)
  size_t tile_cap = 0, scan_cap = 0;
  void* d_tmp = nullptr;        // rocprim's
  size_t tmp_bytes = 0;
  uint32_t* d_irr = nullptr;    // the irregular values of the last format
  uint64_t* h_head = nullptr;   // page-locked {bytes, irregular}
  char* h_text = nullptr;       // page-locked: read's download lands here
  size_t h_text_cap = 0;
  bool formatted = false;       // d_text holds the text of everything appended
};

namespace {
constexpr uint32_t PT_ITEMS = 4, PT_TILE = 256 * PT_ITEMS;
constexpr uint64_t PT_MAX_ROWS = 0xFFFFFFF0ULL;

// EMIT = 0: tile_bytes[t] (and tile_bytes[ntiles] = 0), *irregular.  EMIT = 1: tile_scan in, text out.
// Round j of a block takes the values base + j * 256 + lane: consecutive lanes, consecutive values, so a round's lines are
// consecutive in the text and one block scan per round places them.
template <int EMIT>
__global__ void __launch_bounds__(256) k_predtext(const uint32_t* __restrict__ vals, uint64_t n, uint64_t* __restrict__ tile_bytes,
                                                  const uint64_t* __restrict__ tile_scan, unsigned char* __restrict__ out,
                                                  uint32_t* __restrict__ irregular) {
  using Scan = rocprim::block_scan<uint32_t, 256>;
  using Reduce = rocprim::block_reduce<uint32_t, 256>;
  const uint64_t base = (uint64_t)blockIdx.x * PT_TILE;
  if (!EMIT) {
    __shared__ typename Reduce::storage_type s_red;
    uint32_t bytes = 0, irr = 0;
#pragma unroll
    for (uint32_t j = 0; j < PT_ITEMS; ++j) {
      const uint64_t i = base + j * 256 + threadIdx.x;
      if (i < n) {
        const uint32_t len = dfh_pt::pt_format(vals[i]).len;
        bytes += len;
        irr += len == 0 ? 1u : 0u;
      }
    }
    uint32_t tb = 0, ti = 0;
    Reduce().reduce(bytes, tb, s_red);
    __syncthreads();
    Reduce().reduce(irr, ti, s_red);
    if (threadIdx.x == 0) {
      tile_bytes[blockIdx.x] = tb;
      if (blockIdx.x == 0) tile_bytes[gridDim.x] = 0;
      if (ti) atomicAdd(irregular, ti);
    }
    return;
  }
  __shared__ typename Scan::storage_type s_scan;
  __shared__ __attribute__((aligned(16))) unsigned char img[PT_TILE * dfh_pt::PT_MAX_LINE + 16];
  const uint64_t g_first = tile_scan[blockIdx.x], g_end = tile_scan[blockIdx.x + 1];
  const uint64_t g_img = g_first & ~15ULL;   // the text position of img[0]: a 16 B word of the text is a 16 B word of the image
  uint32_t run = (uint32_t)(g_first - g_img);
#pragma unroll 1
  for (uint32_t j = 0; j < PT_ITEMS; ++j) {
    const uint64_t i = base + j * 256 + threadIdx.x;
    dfh_pt::Line L;
    L.lo = L.hi = 0;
    L.len = 0;
    if (i < n) L = dfh_pt::pt_format(vals[i]);
    uint32_t before = 0, total = 0;
    Scan().exclusive_scan(L.len, before, 0u, total, s_scan);
    unsigned char* p = img + run + before;   // run + before + len <= 15 + PT_TILE * 16
#pragma unroll
    for (uint32_t b = 0; b < 8; ++b)
      if (b < L.len) p[b] = (unsigned char)(L.lo >> (8 * b));
#pragma unroll
    for (uint32_t b = 0; b < 8; ++b)
      if (8 + b < L.len) p[8 + b] = (unsigned char)(L.hi >> (8 * b));
    run += total;
    __syncthreads();   // s_scan is used again; after the last round: the image is complete
  }
  const uint64_t a0 = (g_first + 15) & ~15ULL, a1 = g_end & ~15ULL;   // the aligned words lie in [a0, a1)
  const uint64_t head_end = a0 < g_end ? a0 : g_end;
  for (uint64_t q = g_first + threadIdx.x; q < head_end; q += 256) out[q] = img[q - g_img];
  for (uint64_t q = a0 + 16ULL * threadIdx.x; q < a1; q += 16ULL * 256)
    *reinterpret_cast<uint4*>(out + q) = *reinterpret_cast<const uint4*>(img + (q - g_img));
  for (uint64_t q = (a1 > head_end ? a1 : head_end) + threadIdx.x; q < g_end; q += 256) out[q] = img[q - g_img];
}

void pt_free_retired(dfh_predtext* p) {
  for (void* a : p->retired) (void)hipFree(a);
  p->retired.clear();
}

// room for `extra` more values; the values held so far are copied on the stream, behind the appends that wrote them
int pt_reserve(dfh_predtext* p, size_t extra) {
  const size_t need = p->n + extra;
  if (need <= p->cap) return DFH_OK;
  size_t cap = p->cap ? p->cap : (p->hint ? p->hint : (size_t)1 << 16);
  while (cap < need) cap *= 2;
  float* nv = nullptr;
  if (hipMalloc((void**)&nv, cap * sizeof(float)) != hipSuccess) {
    (void)hipGetLastError();
    set_error("dfh_predtext: no device memory for " + std::to_string(cap) + " values (" + std::to_string(cap * sizeof(float)) +
              " bytes needed)");
    return DFH_ERR_CAPACITY;
  }
  if (p->n) {
    const hipError_t er = hipMemcpyAsync(nv, p->d_val, p->n * sizeof(float), hipMemcpyDeviceToDevice, p->ctx->stream);
    if (er != hipSuccess) {   // the object keeps its array; the new one goes once nothing queued can touch it
      p->retired.push_back(nv);
      set_error(std::string("dfh_predtext: hipMemcpyAsync: ") + hipGetErrorString(er));
      return DFH_ERR_HIP;
    }
  }
  if (p->d_val) p->retired.push_back(p->d_val);
  p->d_val = nv;
  p->cap = cap;
  return DFH_OK;
}

int pt_append(dfh_predtext* p, const float* v, size_t n, hipMemcpyKind kind) {
  if (n == 0) return DFH_OK;
  DFH_HIP(hipSetDevice(p->ctx->device));
  const int rc = pt_reserve(p, n);
  if (rc) return rc;
  DFH_HIP(hipMemcpyAsync(p->d_val + p->n, v, n * sizeof(float), kind, p->ctx->stream));
  p->n += n;
  p->formatted = false;
  return DFH_OK;
}

// a workspace array of at least `count` T (only a format uses them, and the last one has waited for its work)
template <typename T>
int pt_grow(T** ptr, size_t* cap, size_t count, const char* what) {
  if (count <= *cap) return DFH_OK;
  if (*ptr) (void)hipFree(*ptr);
  *ptr = nullptr;
  *cap = 0;
  if (hipMalloc(reinterpret_cast<void**>(ptr), count * sizeof(T)) != hipSuccess) {
    (void)hipGetLastError();
    *ptr = nullptr;
    set_error(std::string("dfh_predtext_format: no device memory for ") + what + " (" + std::to_string(count * sizeof(T)) + " bytes needed)");
    return DFH_ERR_CAPACITY;
  }
  *cap = count;
  return DFH_OK;
}
}  // namespace

extern "C" {

int dfh_predtext_create(dfh_ctx* ctx, size_t capacity_hint, dfh_predtext** out) {
  DFH_ARG(ctx && out, "dfh_predtext_create: NULL argument");
  DFH_ARG(capacity_hint < PT_MAX_ROWS, "dfh_predtext_create: capacity_hint must be below 2^32 - 16 values");
  dfh_predtext* p = new (std::nothrow) dfh_predtext();
  if (!p) {
    set_error("dfh_predtext_create: out of host memory (" + std::to_string(sizeof(dfh_predtext)) + " bytes needed)");
    return DFH_ERR_CAPACITY;
  }
  p->ctx = ctx;
  p->hint = capacity_hint;
  hipError_t e = hipSetDevice(ctx->device);
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&p->d_irr), sizeof(uint32_t));
  if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void**>(&p->h_head), 2 * sizeof(uint64_t), hipHostMallocDefault);
  if (e != hipSuccess) {
    set_error(std::string("dfh_predtext_create: ") + hipGetErrorString(e));
    dfh_predtext_destroy(p);
    return DFH_ERR_HIP;
  }
  *out = p;
  return DFH_OK;
}

int dfh_predtext_destroy(dfh_predtext* p) {
  if (!p) return DFH_OK;
  (void)hipSetDevice(p->ctx->device);
  (void)hipStreamSynchronize(p->ctx->stream);   // queued copies and kernels read and write the arrays
  pt_free_retired(p);
  if (p->d_val) (void)hipFree(p->d_val);
  if (p->d_text) (void)hipFree(p->d_text);
  if (p->d_tile) (void)hipFree(p->d_tile);
  if (p->d_tile_scan) (void)hipFree(p->d_tile_scan);
  if (p->d_tmp) (void)hipFree(p->d_tmp);
  if (p->d_irr) (void)hipFree(p->d_irr);
  if (p->h_head) (void)hipHostFree(p->h_head);
  if (p->h_text) (void)hipHostFree(p->h_text);
  delete p;
  return DFH_OK;
}

int dfh_predtext_reset(dfh_predtext* p) {
  DFH_ARG(p, "dfh_predtext_reset: NULL argument");
  p->n = 0;   // the arrays stay; later appends are queued behind whatever still reads them
  p->formatted = false;
  return DFH_OK;
}

int dfh_predtext_append_batch(dfh_predtext* p, dfh_batch* b) {
  DFH_ARG(p && b, "dfh_predtext_append_batch: NULL argument");
  DFH_ARG(b->ctx == p->ctx, "dfh_predtext_append_batch: the batch belongs to another context");
  DFH_ARG(p->n + (uint64_t)b->nrows < PT_MAX_ROWS, "dfh_predtext_append_batch: the object holds fewer than 2^32 - 16 values");
  // The copy runs on the context's stream, behind the batch's step.  The batch object's NEXT load runs on a preparation stream
  // that waits for ev_free alone, and the step has recorded ev_free already: the hazard dfh_eval_append_batch documents.  The
  // same rule holds here, so that the two calls may follow one step in either order: with pipelining on, ev_free is recorded
  // again behind the copy.  Call it before the next minibatch is loaded into the batch object.
  const int rc = pt_append(p, b->d_pred, b->nrows, hipMemcpyDeviceToDevice);
  if (rc) return rc;
  if (b->nrows && p->ctx->pipeline) {
    DFH_HIP(hipEventRecord(b->ev_free, p->ctx->stream));
    b->free_pending = true;
  }
  return DFH_OK;
}

int dfh_predtext_append_host(dfh_predtext* p, const float* v, size_t n) {
  DFH_ARG(p, "dfh_predtext_append_host: NULL argument");
  DFH_ARG(n < PT_MAX_ROWS && p->n + (uint64_t)n < PT_MAX_ROWS, "dfh_predtext_append_host: the object holds fewer than 2^32 - 16 values");
  DFH_ARG(n == 0 || v, "dfh_predtext_append_host: NULL argument");
  const int rc = pt_append(p, v, n, hipMemcpyHostToDevice);
  if (rc) return rc;
  DFH_HIP(hipStreamSynchronize(p->ctx->stream));   // the caller's array is free on return
  return DFH_OK;
}

int dfh_predtext_count(dfh_predtext* p, uint64_t* n) {
  DFH_ARG(p && n, "dfh_predtext_count: NULL argument");
  *n = p->n;
  return DFH_OK;
}

int dfh_predtext_values(dfh_predtext* p, float* out) {
  DFH_ARG(p && (out || p->n == 0), "dfh_predtext_values: NULL argument");
  DFH_HIP(hipSetDevice(p->ctx->device));
  if (p->n) DFH_HIP(hipMemcpyAsync(out, p->d_val, p->n * sizeof(float), hipMemcpyDeviceToHost, p->ctx->stream));
  DFH_HIP(hipStreamSynchronize(p->ctx->stream));
  pt_free_retired(p);
  return DFH_OK;
}

int dfh_predtext_format(dfh_predtext* p, size_t* nbytes, uint64_t* irregular) {
  DFH_ARG(p && nbytes && irregular, "dfh_predtext_format: NULL argument");
  *nbytes = 0;
  *irregular = 0;
  hipStream_t s = p->ctx->stream;
  DFH_HIP(hipSetDevice(p->ctx->device));
  p->formatted = false;
  p->text_bytes = 0;
  const size_t n = p->n;
  if (n == 0) {
    DFH_HIP(hipStreamSynchronize(s));
    pt_free_retired(p);
    p->formatted = true;
    return DFH_OK;
  }
  const size_t ntiles = (n + PT_TILE - 1) / PT_TILE;
  size_t need = 0;
  DFH_HIP(rocprim::exclusive_scan(nullptr, need, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t)0, ntiles + 1, rocprim::plus<uint64_t>(), s));
  int rc = pt_grow(&p->d_text, &p->text_cap, n * dfh_pt::PT_MAX_LINE, "the text");
  if (!rc) rc = pt_grow(&p->d_tile, &p->tile_cap, ntiles + 1, "the tiles' byte counts");
  if (!rc) rc = pt_grow(&p->d_tile_scan, &p->scan_cap, ntiles + 1, "the tiles' offsets");
  if (!rc) {
    char* tmp = static_cast<char*>(p->d_tmp);
    rc = pt_grow(&tmp, &p->tmp_bytes, std::max<size_t>(need, 256), "the scan");
    p->d_tmp = tmp;
  }
  if (rc) return rc;
  DFH_HIP(hipMemsetAsync(p->d_irr, 0, sizeof(uint32_t), s));
  const uint32_t* vals = reinterpret_cast<const uint32_t*>(p->d_val);
  hipLaunchKernelGGL(k_predtext<0>, dim3((unsigned)ntiles), dim3(256), 0, s, vals, (uint64_t)n, p->d_tile, (const uint64_t*)nullptr,
                     (unsigned char*)nullptr, p->d_irr);
  DFH_HIP(hipGetLastError());
  size_t tb = p->tmp_bytes;
  DFH_HIP(rocprim::exclusive_scan(p->d_tmp, tb, p->d_tile, p->d_tile_scan, (uint64_t)0, ntiles + 1, rocprim::plus<uint64_t>(), s));
  hipLaunchKernelGGL(k_predtext<1>, dim3((unsigned)ntiles), dim3(256), 0, s, vals, (uint64_t)n, (uint64_t*)nullptr, p->d_tile_scan,
                     reinterpret_cast<unsigned char*>(p->d_text), (uint32_t*)nullptr);
  DFH_HIP(hipGetLastError());
  p->h_head[0] = p->h_head[1] = 0;
  DFH_HIP(hipMemcpyAsync(&p->h_head[0], p->d_tile_scan + ntiles, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  DFH_HIP(hipMemcpyAsync(&p->h_head[1], p->d_irr, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  DFH_HIP(hipStreamSynchronize(s));
  pt_free_retired(p);
  p->text_bytes = (size_t)p->h_head[0];
  p->formatted = true;
  *nbytes = p->text_bytes;
  *irregular = p->h_head[1];
  return DFH_OK;
}

int dfh_predtext_read(dfh_predtext* p, char* dst) {
  DFH_ARG(p && (dst || p->text_bytes == 0), "dfh_predtext_read: NULL argument");
  if (!p->formatted) {
    set_error("dfh_predtext_read: nothing formatted (call dfh_predtext_format after the last append)");
    return DFH_ERR_STATE;
  }
  const size_t nb = p->text_bytes;
  if (nb == 0) return DFH_OK;
  DFH_HIP(hipSetDevice(p->ctx->device));
  if (nb > p->h_text_cap) {   // the download lands in page-locked memory of the object's, kept
    if (p->h_text) DFH_HIP(hipHostFree(p->h_text));
    p->h_text = nullptr;
    p->h_text_cap = 0;
    const size_t c = nb + nb / 4;
    DFH_HIP(hipHostMalloc(reinterpret_cast<void**>(&p->h_text), c, hipHostMallocDefault));
    p->h_text_cap = c;
  }
  DFH_HIP(hipMemcpyAsync(p->h_text, p->d_text, nb, hipMemcpyDeviceToHost, p->ctx->stream));
  DFH_HIP(hipStreamSynchronize(p->ctx->stream));
  memcpy(dst, p->h_text, nb);
  return DFH_OK;
}

int dfh_predtext_tile(void) { return (int)PT_TILE; }

}  // extern "C"
