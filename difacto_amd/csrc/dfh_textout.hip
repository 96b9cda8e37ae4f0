// dfh_textout.hip — what the device formatters share (dfh_predtext.hip, dfh_dumptext.hip, dfh_listtext.hip): everything of a
// format that is not a line's own arithmetic.  A formatter turns ROWS (values, entries, lists) into the bytes fprintf would write,
// concatenated in order, in two passes over tiles of T rows, a block of 256 threads per tile:
//   measure (EMIT = 0)  each row's length (kept in rlen, 4 B per row, where the formatter carries them between the passes), the
//                       tile's bytes, and the values the arithmetic does not format added to the one counter the blocks share (an
//                       atomic per block that has any)
//   rocprim::exclusive_scan over the tiles' bytes (and a 0 behind them: the last offset is all bytes)
//   emit (EMIT = 1)     the rows are formatted ONCE MORE into an LDS image of the tile's text at their scanned offsets, the image
//                       shifted by the tile's first byte mod 16; then the block writes the image with aligned 16 B stores, and
//                       only the tile's unaligned head and tail byte by byte (two neighbouring tiles meet inside one 16 B word:
//                       each writes its own bytes of it)
// and {bytes, irregular[, a counter of the caller's]} are read back: one host round trip.  The launches are ordered by the stream
// alone: no block waits for another.  Plain C++, vector stores, no scratch.
// Host side: TextWork, the workspace an object keeps (to_release); dev_grow, the workspace arrays' growth; to_format, the two
// passes around the scan; to_read, the text's download.  Device side: to_tile_begin (the emit pass's prologue), to_measure_begin /
// to_measure_end / to_tile_out (what the measure pass leaves), to_group_scan (a row's lanes), to_store (the image's way out).
namespace {
// the LDS image of a tile's text (and 16 B for its shift); rows per tile at most, where rows' lengths are carried: 4 per thread
constexpr uint32_t TO_IMG = 32768, TO_TILE_MAX = 1024;

// an array of at least `count` T that only grows and keeps nothing (the call that used it last has waited for its work)
template <typename T>
int dev_grow(T** ptr, size_t* cap, size_t count, const char* who, const char* what) {
  if (count <= *cap) return DFH_OK;
  if (*ptr) (void)hipFree(*ptr);
  *ptr = nullptr;
  *cap = 0;
  if (hipMalloc(reinterpret_cast<void**>(ptr), count * sizeof(T)) != hipSuccess) {
    (void)hipGetLastError();
    *ptr = nullptr;
    set_error(std::string(who) + ": no device memory for " + what + " (" + std::to_string(count * sizeof(T)) + " bytes needed)");
    return DFH_ERR_CAPACITY;
  }
  *cap = count;
  return DFH_OK;
}

// a formatter's workspace, grown to what a format needs, kept with its object
struct TextWork {
  char* d_text = nullptr;         // [text_cap] the text of the last format
  size_t text_cap = 0, text_bytes = 0;
  uint32_t* d_rlen = nullptr;     // [rlen_cap] bytes per row of the unit (formatters that carry them)
  size_t rlen_cap = 0;
  uint64_t *d_tile = nullptr, *d_tile_scan = nullptr;   // bytes per tile (and a 0), their exclusive scan (the last: all bytes)
  size_t tile_cap = 0, scan_cap = 0;
  char* d_tmp = nullptr;          // rocprim's
  size_t tmp_bytes = 0;
  uint32_t* d_irr = nullptr;      // the irregular values of the last format; made by the first format, like h_head
  uint64_t* h_head = nullptr;     // page-locked {bytes, irregular, the caller's counter}
  char* h_text = nullptr;         // page-locked: to_read's download lands here
  size_t h_text_cap = 0;
  uint64_t nonfinite = 0;         // the caller's counter as the last format read it back
};

void to_release(TextWork* w) {
  if (w->d_text) (void)hipFree(w->d_text);
  if (w->d_rlen) (void)hipFree(w->d_rlen);
  if (w->d_tile) (void)hipFree(w->d_tile);
  if (w->d_tile_scan) (void)hipFree(w->d_tile_scan);
  if (w->d_tmp) (void)hipFree(w->d_tmp);
  if (w->d_irr) (void)hipFree(w->d_irr);
  if (w->h_head) (void)hipHostFree(w->h_head);
  if (w->h_text) (void)hipHostFree(w->h_text);
  *w = TextWork();
}

// what a pass's launch gets from the workspace; what a pass does not use is NULL
struct TextPass {
  uint32_t* rlen;
  uint64_t* tile_bytes;
  const uint64_t* tile_scan;
  unsigned char* out;
  uint32_t* irregular;
};

// Formats `rows` rows in tiles of `tile`, none longer than max_line bytes: launch(emit, ntiles, TextPass) queues pass 0 and pass
// 1 on the context's stream.  d_nf (or NULL): a 64-bit device counter read back with the head, into w->nonfinite.  One wait, also
// for no rows.  The caller has set the device and cleared its `formatted`, and sets it on DFH_OK.
template <typename Launch>
int to_format(dfh_ctx* c, TextWork* w, size_t rows, uint32_t tile, size_t max_line, bool row_lens, const unsigned long long* d_nf,
              const char* who, Launch&& launch, size_t* nbytes, uint64_t* irregular) {
  hipStream_t s = c->stream;
  w->text_bytes = 0;
  w->nonfinite = 0;
  hipError_t e = hipSuccess;
  if (!w->d_irr) e = hipMalloc(reinterpret_cast<void**>(&w->d_irr), sizeof(uint32_t));
  if (e == hipSuccess && !w->h_head) e = hipHostMalloc(reinterpret_cast<void**>(&w->h_head), 3 * sizeof(uint64_t), hipHostMallocDefault);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    set_error(std::string(who) + ": " + hipGetErrorString(e));
    return DFH_ERR_HIP;
  }
  w->h_head[0] = w->h_head[1] = w->h_head[2] = 0;
  if (rows) {
    const size_t ntiles = (rows + tile - 1) / tile;
    size_t need = 0;
    DFH_HIP(rocprim::exclusive_scan(nullptr, need, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t)0, ntiles + 1, rocprim::plus<uint64_t>(), s));
    int rc = dev_grow(&w->d_text, &w->text_cap, rows * max_line, who, "the text");
    if (!rc && row_lens) rc = dev_grow(&w->d_rlen, &w->rlen_cap, rows, who, "the rows' byte counts");
    if (!rc) rc = dev_grow(&w->d_tile, &w->tile_cap, ntiles + 1, who, "the tiles' byte counts");
    if (!rc) rc = dev_grow(&w->d_tile_scan, &w->scan_cap, ntiles + 1, who, "the tiles' offsets");
    if (!rc) rc = dev_grow(&w->d_tmp, &w->tmp_bytes, std::max<size_t>(need, 256), who, "the scan");
    if (rc) return rc;
    DFH_HIP(hipMemsetAsync(w->d_irr, 0, sizeof(uint32_t), s));
    launch(0, (unsigned)ntiles, TextPass{w->d_rlen, w->d_tile, nullptr, nullptr, w->d_irr});
    DFH_HIP(hipGetLastError());
    size_t tb = w->tmp_bytes;
    DFH_HIP(rocprim::exclusive_scan(w->d_tmp, tb, w->d_tile, w->d_tile_scan, (uint64_t)0, ntiles + 1, rocprim::plus<uint64_t>(), s));
    launch(1, (unsigned)ntiles, TextPass{w->d_rlen, nullptr, w->d_tile_scan, reinterpret_cast<unsigned char*>(w->d_text), nullptr});
    DFH_HIP(hipGetLastError());
    DFH_HIP(hipMemcpyAsync(&w->h_head[0], w->d_tile_scan + ntiles, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    DFH_HIP(hipMemcpyAsync(&w->h_head[1], w->d_irr, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  }
  if (d_nf) DFH_HIP(hipMemcpyAsync(&w->h_head[2], d_nf, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  DFH_HIP(hipStreamSynchronize(s));
  w->text_bytes = (size_t)w->h_head[0];
  w->nonfinite = w->h_head[2];
  *nbytes = w->text_bytes;
  *irregular = w->h_head[1];
  return DFH_OK;
}

// the text of the last format into dst, through page-locked memory of the object's, kept; the caller has checked its state
int to_read(dfh_ctx* c, TextWork* w, char* dst) {
  const size_t nb = w->text_bytes;
  if (nb == 0) return DFH_OK;
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

using TextScan = rocprim::block_scan<uint32_t, 256>;

// where a tile's text lies: bytes [g_first, g_end) of the text; g_img: the text position of img[0] (a 16 B word of the text is
// a 16 B word of the image); run0: where the tile's first byte sits in the image
struct TextTile {
  uint64_t g_first, g_end, g_img;
  uint32_t run0;
};

// The emit pass's prologue, by the whole block: the lengths of the tile's tn <= TO_TILE_MAX rows (rlen[base ..]) scanned into
// s_off[TO_TILE_MAX], where each row's line starts in the tile's text, and the tile's place.  Synchronised on return.
__device__ __forceinline__ TextTile to_tile_begin(const uint32_t* __restrict__ rlen, uint64_t base, uint32_t tn,
                                                  const uint64_t* __restrict__ tile_scan, uint32_t* s_off,
                                                  typename TextScan::storage_type& s_scan) {
  uint32_t len4[4], off4[4];
#pragma unroll
  for (uint32_t i = 0; i < 4; ++i) {
    const uint32_t r = 4 * threadIdx.x + i;
    len4[i] = r < tn ? rlen[base + r] : 0u;
  }
  TextScan().exclusive_scan(len4, off4, 0u, s_scan);
#pragma unroll
  for (uint32_t i = 0; i < 4; ++i) s_off[4 * threadIdx.x + i] = off4[i];   // 4 * 256 = TO_TILE_MAX
  TextTile t;
  t.g_first = tile_scan[blockIdx.x];
  t.g_end = tile_scan[blockIdx.x + 1];
  t.g_img = t.g_first & ~15ULL;
  t.run0 = (uint32_t)(t.g_first - t.g_img);
  __syncthreads();
  return t;
}

// what the measure pass leaves of a tile, by one thread of its block: its bytes (block 0: and the 0 behind the last tile's) and
// its irregular values
__device__ __forceinline__ void to_tile_out(uint32_t bytes, uint32_t irr, uint64_t* __restrict__ tile_bytes, uint32_t* __restrict__ irregular) {
  tile_bytes[blockIdx.x] = bytes;
  if (blockIdx.x == 0) tile_bytes[gridDim.x] = 0;
  if (irr) atomicAdd(irregular, irr);
}

// s_acc[2]: the tile's bytes (a row's first lane adds its line's to s_acc[0]) and its irregular values
__device__ __forceinline__ void to_measure_begin(uint32_t* s_acc) {
  if (threadIdx.x < 2) s_acc[threadIdx.x] = 0;
  __syncthreads();
}

__device__ __forceinline__ void to_measure_end(uint32_t* s_acc, uint32_t irr, uint64_t* __restrict__ tile_bytes, uint32_t* __restrict__ irregular) {
  if (irr) atomicAdd(&s_acc[1], irr);
  __syncthreads();
  if (threadIdx.x == 0) to_tile_out(s_acc[0], s_acc[1], tile_bytes, irregular);
}

// inclusive scan of x inside a row's P lanes (a power of two <= 64; g: the lane in its group, lead: the group's first lane of the
// wave); *total: the group's sum.  All 64 lanes call it.
__device__ __forceinline__ uint32_t to_group_scan(uint32_t x, uint32_t P, uint32_t g, uint32_t lead, uint32_t* total) {
  for (uint32_t o = 1; o < P; o <<= 1) {
    const uint32_t y = (uint32_t)__shfl_up((int)x, o, 64);
    if (g >= o) x += y;
  }
  *total = (uint32_t)__shfl((int)x, (int)(lead + P - 1u), 64);
  return x;
}

// The emit pass's end, by the whole block, once the image is complete (the caller has synchronised): bytes [g_first, g_end) of
// the text out of img, whose byte 0 is the text's byte g_img = g_first & ~15.
__device__ __forceinline__ void to_store(unsigned char* __restrict__ out, const unsigned char* img, uint64_t g_first, uint64_t g_end, uint64_t g_img) {
  const uint64_t a0 = (g_first + 15) & ~15ULL, a1 = g_end & ~15ULL;   // the aligned words lie in [a0, a1)
  const uint64_t head_end = a0 < g_end ? a0 : g_end;
  for (uint64_t q = g_first + threadIdx.x; q < head_end; q += 256) out[q] = img[q - g_img];
  for (uint64_t q = a0 + 16ULL * threadIdx.x; q < a1; q += 16ULL * 256)
    *reinterpret_cast<uint4*>(out + q) = *reinterpret_cast<const uint4*>(img + (q - g_img));
  for (uint64_t q = (a1 > head_end ? a1 : head_end) + threadIdx.x; q < g_end; q += 256) out[q] = img[q - g_img];
}
}  // namespace
