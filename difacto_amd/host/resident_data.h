/**
 * resident_data.h — how learner = lbfgs and learner = bcd cut what their readers give into the chunks they keep in HBM
 * (dfh_lbfgs_add_chunk / dfh_bcd_add_chunk).  Their common way out, SaveDenseModel, is in model_parts.h.
 */
#ifndef DIFACTO_HOST_RESIDENT_DATA_H_
#define DIFACTO_HOST_RESIDENT_DATA_H_
#include <cstddef>

namespace difacto {

/*! \brief the entries a resident chunk may hold: the batch object's positions are 32 bits */
constexpr size_t kMaxChunkNnz = size_t(1) << 31;

/*! \brief every block of the reader as chunks of whole rows: fn(r0, r1, blk) for rows [r0, r1) of blk, cut so that no
 * chunk holds more than max_nnz entries (a single row beyond it is passed on alone, for add_chunk to refuse) */
template <typename ReaderT, typename Fn>
inline void ForEachChunk(ReaderT* reader, size_t max_nnz, Fn fn) {
  while (reader->Next()) {
    const auto& blk = reader->Value();
    for (size_t r0 = 0; r0 < blk.size;) {
      size_t r1 = r0 + 1;
      while (r1 < blk.size && blk.offset[r1 + 1] - blk.offset[r0] <= max_nnz) ++r1;
      fn(r0, r1, blk);
      r0 = r1;
    }
  }
}

}  // namespace difacto
#endif  // DIFACTO_HOST_RESIDENT_DATA_H_
