/**
 * sgd_data_cache.h — data_cache = hbm of the SGD learner: the parsed rows of a data part stay in device memory.
 *
 * The device feed (device_feed.h) uploads the reader's shuffle buffers into device row buffers (dfh_rowbuf) and recycles
 * them.  With the cache the buffers of a job part — (job type, part) — are KEPT, in the order the reader built them, each
 * with what the host still needs of it: its row offsets (the minibatch boundaries by nnz, the size of the batch objects)
 * and its labels (negative down-sampling tests them), 12 B per row.  The ids and values — everything the parser produced,
 * ~300 B per criteo row — exist in HBM only.  In a later epoch the part's BatchReader takes its shuffle buffers from here
 * (CachedBuffers below) instead of from a Reader: no file is opened, no parser thread started, nothing uploaded; the
 * permutation, the sampling draws and the minibatch boundaries are BatchReader::Next's own, so the minibatches are the ones
 * an uncached run cuts.
 */
#ifndef DIFACTO_HOST_SGD_DATA_CACHE_H_
#define DIFACTO_HOST_SGD_DATA_CACHE_H_
#include <map>
#include <memory>
#include <utility>
#include <vector>
#include "./batch_reader.h"
#include "difacto_hip.h"

namespace difacto {

/*! \brief one shuffle buffer that stays: the device rows, and the host's description of them */
struct CachedBuffer {
  dfh_rowbuf* rb = nullptr;
  std::vector<size_t> offset;   // [rows + 1], from 0
  std::vector<real_t> label;    // [rows]
  size_t bytes = 0;             // device bytes the buffer holds
};

/*! \brief the buffers of one job part, serial 1, 2, .. = bufs[0], bufs[1], .. */
struct CachedPart {
  std::vector<CachedBuffer> bufs;
  size_t rows = 0, bytes = 0;
  ~CachedPart() {
    for (auto& b : bufs)
      if (b.rb) dfh_rowbuf_destroy(b.rb);
  }
};

/*! \brief what the learner keeps: the parts that fitted, and the parts that did not (they are not tried again) */
struct SGDDataCache {
  std::map<std::pair<int, int>, std::unique_ptr<CachedPart>> parts;   // (job type, part_idx)
  std::map<std::pair<int, int>, bool> refused;
  size_t bytes = 0;
  const CachedPart* Find(int job_type, int part) const {
    auto it = parts.find(std::make_pair(job_type, part));
    return it == parts.end() ? nullptr : it->second.get();
  }
};

/*! \brief BatchReader's second source of shuffle buffers: the cached ones, in order (offsets and labels; the rows are on the
 *  device, named by the buffer's serial) */
class CachedBuffers : public BatchSource {
 public:
  explicit CachedBuffers(const CachedPart* part) : part_(part) {}
  bool Next() override {
    if (next_ >= part_->bufs.size()) return false;
    const CachedBuffer& b = part_->bufs[next_++];
    blk_ = dmlc::RowBlock<feaid_t>();
    blk_.size = b.label.size();
    blk_.offset = b.offset.data();
    blk_.label = b.label.data();
    blk_.weight = nullptr;
    blk_.index = nullptr;
    blk_.value = nullptr;
    return true;
  }
  const dmlc::RowBlock<feaid_t>& Value() const override { return blk_; }
  void MoveOut(RowChunk* dst) override { LOG(FATAL) << "a cached buffer stays where it is"; }

 private:
  const CachedPart* part_;
  size_t next_ = 0;
  dmlc::RowBlock<feaid_t> blk_;
};

}  // namespace difacto
#endif  // DIFACTO_HOST_SGD_DATA_CACHE_H_
