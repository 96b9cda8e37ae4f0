// The page-locked staging block of a batch object and the tile-row table of a described minibatch: plain host code, no HIP
// types, so the host-side tests include it.  The device reads this block IN PLACE through a mapped pointer (k_loc_describe,
// k_loc_count_gather, k_gather_rows_staged): every path that writes it takes its offsets from StageLayout.
#ifndef DFH_FEED_LAYOUT_H_
#define DFH_FEED_LAYOUT_H_
#include <stddef.h>
#include <stdint.h>

namespace dfh {

#ifndef DFH_LOC_TILE
#define DFH_LOC_TILE 2048
#endif
constexpr int LOC_TILE = DFH_LOC_TILE;  // pairs per block in the Localizer's count / scatter passes
constexpr int LOC_GATHER_ROWS = 1024;   // rows a tile may span (the host checks; beyond: the gather runs as its own launch)
constexpr int LOC_GATHER_SEGS = 4;      // row buffers one minibatch may draw from
constexpr int LOC_DESC_ROWS = 256;      // rows per block of k_loc_describe

//   offsets [max_rows + 1] | labels [max_rows] | (256 B aligned) ids [max_nnz] u64 | values [max_nnz]      dfh_batch_load_host
//   offsets                | labels            | row numbers [max_rows + 1] u32 | tile rows [max_tiles + 2] | block bases
// A described minibatch (dfh_batch_gather_rows, _prepare_rows, _prepare_cached) puts its row numbers where load_host puts the
// ids, the first row of every tile behind them and, cached only, k_loc_describe's block bases behind those.
struct StageLayout {
  size_t o_off = 0, o_lab = 0, o_idx = 0, o_val = 0, o_tile = 0, o_base = 0, load_host_bytes = 0;
  StageLayout() {}
  StageLayout(size_t max_rows, size_t max_nnz, size_t max_tiles) {
    o_lab = (max_rows + 1) * 4;
    o_idx = (o_lab + max_rows * 4 + 255) & ~(size_t)255;
    o_val = o_idx + max_nnz * 8;
    load_host_bytes = o_val + max_nnz * 4;
    o_tile = o_idx + (max_rows + 1) * 4;
    o_base = o_tile + (max_tiles + 2) * 4;
  }
  size_t rows_bytes() const { return o_base; }                                // through the tile rows
  size_t cached_bytes(size_t nblk) const { return o_base + (nblk + 1) * 4; }  // through nblk + 1 block bases
};

// h_tile[t] = the last row that starts at or before position t * LOC_TILE, for every tile of a minibatch of nrows rows with
// the cumulative offsets off[0 .. nrows]; returns the number of tiles
inline size_t tile_rows_fill(const uint32_t* off, size_t nrows, uint32_t* h_tile) {
  const size_t ntiles = ((size_t)off[nrows] + LOC_TILE - 1) / LOC_TILE;
  size_t r = 0;
  for (size_t t = 0; t < ntiles; ++t) {
    const uint32_t p = (uint32_t)(t * LOC_TILE);
    while (r + 1 < nrows && off[r + 1] <= p) ++r;
    h_tile[t] = (uint32_t)r;
  }
  return ntiles;
}

// Can the count pass gather this minibatch itself?  It has pairs, draws from at most LOC_GATHER_SEGS buffers, and no tile
// (the last one with the trailing empty rows included) spans more than LOC_GATHER_ROWS rows.  Writes the sentinel
// h_tile[ntiles] = nrows of a table the count pass will read.
inline bool tile_rows_finish(uint32_t* h_tile, size_t ntiles, size_t nrows, size_t nnz, size_t nsegs_used) {
  if (nnz == 0 || nsegs_used > (size_t)LOC_GATHER_SEGS) return false;
  for (size_t q = 1; q < ntiles; ++q)
    if ((size_t)h_tile[q] - h_tile[q - 1] + 1 > (size_t)LOC_GATHER_ROWS) return false;
  h_tile[ntiles] = (uint32_t)nrows;
  return nrows - h_tile[ntiles - 1] <= (size_t)LOC_GATHER_ROWS;
}

}  // namespace dfh
#endif  // DFH_FEED_LAYOUT_H_
