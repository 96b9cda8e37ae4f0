// dfh_predtext.hip — prediction text on the device: the bytes fprintf("%.9g\n", v) writes for every prediction appended since
// the last reset, concatenated in order (included at the end of dfh_api.hip; the learner's pred_write = device).  Modelled on
// dfh_eval.hip for everything but the arithmetic: the appended values sit in one device array that grows by doubling, appends
// are copies queued on the context's stream, a replaced array is freed behind the next wait.
// The arithmetic is dfh_predtext_fmt.h: exact, integer only, for the REGULAR values (+-0 and 2^-64 <= |v| < 2^32).  Anything
// else is counted, and the caller formats such a set on the host — the idiom of the parse and decode kernels.
// dfh_predtext_format is the two passes of dfh_textout.hip with k_predtext: a tile is PT_TILE values, a lane per value and round,
// and NO per-value length is carried between the passes: the emit pass formats the lines once more and places a round's lines
// with one block scan (a 16 B slot per value would cost 33 B of traffic per value to save ~250 integer instructions; 4 B per
// value would still be a write and a read that the scan makes unnecessary).  Its image is PT_TILE * 16 + 16 bytes.  These
// kernels are not in the timing registry (dfh_kernel_name) and no launch of a step changes.
#include "dfh_predtext_fmt.h"

struct dfh_predtext {
  dfh_ctx* ctx = nullptr;
  float* d_val = nullptr;       // [cap] the appended values
  size_t cap = 0, n = 0, hint = 0;
  std::vector<void*> retired;   // arrays a growth replaced: copies out of them may still be queued, freed behind the next wait
  TextWork text;                // format's workspace (dfh_textout.hip)
  bool formatted = false;       // text holds the text of everything appended
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
    if (threadIdx.x == 0) to_tile_out(tb, ti, tile_bytes, irregular);
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
    dfh_pt::pt_put(img + run + before, L.lo, L.hi, L.len);   // run + before + len <= 15 + PT_TILE * 16
    run += total;
    __syncthreads();   // s_scan is used again; after the last round: the image is complete
  }
  to_store(out, img, g_first, g_end, g_img);
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
  *out = p;
  return DFH_OK;
}

int dfh_predtext_destroy(dfh_predtext* p) {
  if (!p) return DFH_OK;
  (void)hipSetDevice(p->ctx->device);
  (void)hipStreamSynchronize(p->ctx->stream);   // queued copies and kernels read and write the arrays
  pt_free_retired(p);
  if (p->d_val) (void)hipFree(p->d_val);
  to_release(&p->text);
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
  const uint32_t* vals = reinterpret_cast<const uint32_t*>(p->d_val);
  const uint64_t n = p->n;
  const int rc = to_format(p->ctx, &p->text, p->n, PT_TILE, dfh_pt::PT_MAX_LINE, false, nullptr, "dfh_predtext_format",
                           [&](int emit, unsigned ntiles, const TextPass& a) {
                             hipLaunchKernelGGL(emit ? k_predtext<1> : k_predtext<0>, dim3(ntiles), dim3(256), 0, s, vals, n, a.tile_bytes,
                                                a.tile_scan, a.out, a.irregular);
                           },
                           nbytes, irregular);
  if (rc) return rc;
  pt_free_retired(p);   // behind the format's wait
  p->formatted = true;
  return DFH_OK;
}

int dfh_predtext_read(dfh_predtext* p, char* dst) {
  DFH_ARG(p && (dst || p->text.text_bytes == 0), "dfh_predtext_read: NULL argument");
  if (!p->formatted) {
    set_error("dfh_predtext_read: nothing formatted (call dfh_predtext_format after the last append)");
    return DFH_ERR_STATE;
  }
  return to_read(p->ctx, &p->text, dst);
}

int dfh_predtext_tile(void) { return (int)PT_TILE; }

}  // extern "C"
