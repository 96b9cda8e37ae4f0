/**
 * bcd_learner.h — BCDLearner: the reference's block coordinate descent learner (src/bcd/bcd_learner.{h,cc}) with the
 * training and validation data, the predictions and the model resident in HBM (dfh_bcd, include/difacto_hip.h).
 *
 * The scheduler loop (RunScheduler: load, feature-group statistics, PartitionFeature, the shuffled epochs, the epoch-end
 * callbacks and the log line) follows bcd_learner.cc:51-92.  The jobs it issues there to workers and servers are calls
 * on one dfh_bcd object here: one process, one GPU, one host call per epoch.
 *
 * Differences from the reference:
 *   - no tile store on disk (data_cache is accepted and unused)
 *   - g and h are summed in fp64 (the reference adds floats in row order): the same objective to ~1e-6
 *   - model_out is written (the reference declares it and never writes it): the final w in the format of learner = sgd's
 *     model_out, without optimiser state, so that task = predict learner = sgd model_in = ... V_dim = 0 scores it
 *   - model_in is read (the reference declares it, bcd_param.h:44, and never reads it): a warm start from the w of a model
 *     file of any learner (V and optimiser state in the file are ignored), e.g. the previous l1 of a regularisation
 *     path; keys the feature map does not hold are dropped, delta starts at 1 as in a cold run
 *   - a sharded store (DMLC_ROLE / DMLC_NUM_WORKER > 1) is refused with a message; so is task = predict for a caller of
 *     Learner::Create("bcd") (the command line scores a model through learner = sgd's prediction path itself)
 *   - shard_rows = 1 (default 0) with the complete environment of a rank (DMLC_ROLE=worker, DMLC_NUM_WORKER, DIFACTO_RANK,
 *     DIFACTO_RENDEZVOUS): one process per GPU.  Every rank reads part rank of the rows, holds the whole model and runs
 *     this scheduler loop itself on its own RefRand stream (same seed, same block order); the reference's worker and
 *     server jobs of a block are the stages of dfh_bcd_create_sharded's block step.  The feature-group statistics and
 *     the progress are summed over the ranks in rank order, so every rank prints the same lines; rank 0 alone writes
 *     model_out, as one file.  Without the complete environment shard_rows = 1 is refused, naming what is missing.
 */
#ifndef DIFACTO_HOST_BCD_LEARNER_H_
#define DIFACTO_HOST_BCD_LEARNER_H_
#include <functional>
#include <string>
#include <utility>
#include <vector>
#include <memory>
#include "./bcd_param.h"
#include "./comm_setup.h"
#include "difacto/learner.h"
#include "difacto_hip.h"

namespace difacto {
namespace bcd {

/*! \brief a key range [begin, end) (src/common/range.h:11-60) */
struct Range {
  uint64_t begin = 0, end = 0;
  Range() {}
  Range(uint64_t b, uint64_t e) : begin(b), end(e) {}
  /*! \brief Range::Segment (range.h:19-29): the idx-th of nparts, in the reference's double arithmetic */
  Range Segment(uint64_t idx, uint64_t nparts) const {
    const double itv = static_cast<double>(end - begin) / static_cast<double>(nparts);
    const uint64_t b = static_cast<uint64_t>(begin + itv * idx);
    const uint64_t e = (idx == nparts - 1) ? end : static_cast<uint64_t>(begin + itv * (idx + 1));
    return Range(b, e);
  }
  bool Valid() const { return end > begin; }
};

/*! \brief PartitionFeature (bcd_utils.h:65-89): the ReverseBytes key space of each (group, #blocks) cut into ranges */
void PartitionFeature(int feagrp_nbits, const std::vector<std::pair<int, int>>& feagrps, std::vector<Range>* feablks);

/*! \brief FeaGroupStats (bcd_utils.h:92-131): per group the entries of every 10th row of each chunk, then the rows
 * counted and all rows */
class FeaGroupStats {
 public:
  explicit FeaGroupStats(int nbits);
  void Add(size_t nrows, const size_t* offset, const feaid_t* index);
  void Get(std::vector<real_t>* value) const { *value = value_; }

 private:
  int nbits_;
  int skip_ = 10;
  std::vector<real_t> value_;
};

}  // namespace bcd

class BCDLearner : public Learner {
 public:
  BCDLearner() {}
  virtual ~BCDLearner();
  KWArgs Init(const KWArgs& kwargs) override;

  void AddEpochEndCallback(const std::function<void(int epoch, const std::vector<real_t>& prog)>& callback) {
    epoch_end_callback_.push_back(callback);
  }
  /*! \brief rows of every training chunk, in order (known after Run) */
  const std::vector<size_t>& train_chunk_rows() const { return chunk_rows_; }

 protected:
  void RunScheduler() override;
  void Process(const std::string& args, std::string* rets) override {}

 private:
  /*! \brief PrepareData (bcd_learner.cc:96-131): the chunks onto the device, the feature-group statistics */
  void PrepareData(std::vector<real_t>* fea_stats);
  /*! \brief model_in: warm start from a model file (dfh_bcd_set_model), after the feature map is built */
  void LoadModel(uint64_t nkeys);
  void SaveModel();

  BCDLearnerParam param_;
  BCDUpdaterParam updater_param_;
  dfh_bcd* obj_ = nullptr;
  // shard_rows = 1: this rank's place and the communicator (comm_setup.h)
  dfh_comm* comm_ = nullptr;
  std::unique_ptr<FileExchange> files_;
  int rank_ = 0, world_ = 1;
  std::vector<size_t> chunk_rows_;
  std::vector<std::function<void(int epoch, const std::vector<real_t>& prog)>> epoch_end_callback_;
};

}  // namespace difacto
#endif  // DIFACTO_HOST_BCD_LEARNER_H_
