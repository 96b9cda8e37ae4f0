/**
 * sgd_learner.h — SGDLearner: the reference's SGD learner (src/sgd/sgd_learner.{h,cc})
 * with its worker loop running on the GPU.
 *
 * Scheduler side (epochs, job issue, progress merge, stop criteria, epoch-end
 * callbacks) follows the reference line by line.  The worker loop
 * IterateData has two implementations, chosen by the `device_path` key:
 *
 *   fused   (default) every minibatch goes to the device as raw CSR; Localizer,
 *           Pull, Predict, Evaluate, CalcGrad, Push and the FTRL/AdaGrad update
 *           run there (dfh_localize / dfh_sgd_step); batch t+1 is prepared on a
 *           second stream while batch t trains — the overlap the reference gets
 *           from its reader thread + batch tracker (sgd_learner.cc:196-224)
 *   literal the reference's own sequence of interface calls with host arrays:
 *           Localizer::Compact -> Store::Push(kFeaCount) -> Store::Pull ->
 *           GetPos -> Loss::Predict -> Loss::Evaluate -> Loss::CalcGrad ->
 *           Store::Push(kGradient), each served by the device adaptors
 */
#ifndef DIFACTO_HOST_SGD_LEARNER_H_
#define DIFACTO_HOST_SGD_LEARNER_H_
#include <cstdio>
#include <functional>
#include <future>
#include <string>
#include <vector>
#include "./batch_ring.h"
#include "./device_store.h"
#include "./sgd_data_cache.h"
#include "./sgd_loop_env.h"
#include "./sgd_param.h"
#include "./sgd_utils.h"
#include "difacto/learner.h"
#include "difacto/loss.h"
#include "difacto/store.h"

namespace difacto {
struct DeviceFeed;
struct DeviceTextParse;
struct DeviceRecDecode;

class SGDLearner : public Learner {
 public:
  SGDLearner() : store_(nullptr), loss_(nullptr) {}
  virtual ~SGDLearner();

  KWArgs Init(const KWArgs& kwargs) override;

  /*! \brief called after every epoch with the merged training / validation progress */
  void AddEpochEndCallback(const std::function<void(int epoch, const sgd::Progress& train, const sgd::Progress& val)>& cb) {
    epoch_end_callback_.push_back(cb);
  }
  DeviceSGDUpdater* GetUpdater() {
    return CHECK_NOTNULL(static_cast<DeviceSGDUpdater*>(CHECK_NOTNULL(store_)->updater().get()));
  }

 protected:
  void RunScheduler() override;
  void Process(const std::string& args, std::string* rets) override;

 private:
  void RunEpoch(int epoch, int job_type, sgd::Progress* prog);
  /*! \brief task = predict: one forward pass of the loaded model over the data, predictions to pred_out */
  void RunPrediction();
  /*! \brief prediction jobs: the step's logits, one line per example, appended to the job's output file */
  void WritePredictions(dfh_batch* b);
  /*! \brief pred_write = device: the unit's predictions become text on the device (or, a unit the device does not format, on
   *  the host) and go to the job's output file, behind the unit before it; the unit starts empty again */
  void ClosePredUnit();
  /*! \brief pred_write = device: waits for the unit that is still being written */
  void WaitPredWrite();
  /*! \brief exact_metrics = 1: the whole-set figures of the pass that has just ended, as one log line behind `what` */
  void LogExactMetrics(const char* what);
  /*! \brief the data a job reads: data_in for training, data_val for validation, either for prediction */
  const std::string& JobData(const sgd::Job& job) const;
  void IterateData(const sgd::Job& job, sgd::Progress* prog);
  // the fused loop (sgd_learner.cc): what the job reads from, its reader, the prepare / step loop, the cache's bookkeeping
  void IterateDataFused(const sgd::Job& job, sgd::Progress* prog);
  struct FusedSource;
  FusedSource SourceOf(const sgd::Job& job, const SgdLoopEnv& env);
  BatchReader* NewFusedReader(const sgd::Job& job, const FusedSource& src, const SgdLoopEnv& env, DeviceFeed* feed,
                              DeviceTextParse* text_parse, DeviceRecDecode* rec_decode);
  void RunFused(const sgd::Job& job, const FusedSource& src, const SgdLoopEnv& env, BatchSource* reader, DeviceFeed* feed,
                sgd::Progress* prog);
  void CloseCachedJob(const sgd::Job& job, const FusedSource& src, DeviceFeed* feed);
  void IterateDataLiteral(const sgd::Job& job, sgd::Progress* prog);
  void IterateDataSharded(const sgd::Job& job, sgd::Progress* prog);
  /*! \brief sums the record over the ranks of a sharded run (identity for one process) */
  void MergeAcrossRanks(sgd::Progress* prog);
  real_t EvaluatePenalty(const SArray<real_t>& weights, const SArray<int>& w_pos, const SArray<int>& V_pos);
  void GetPos(const SArray<int>& len, SArray<int>* w_pos, SArray<int>* V_pos);
  void SaveModel();
  void LoadModel();

  Store* store_;
  Loss* loss_;
  SGDLearnerParam param_;
  int blk_nthreads_ = DEFAULT_NTHREADS;
  std::vector<std::function<void(int, const sgd::Progress&, const sgd::Progress&)>> epoch_end_callback_;
  BatchRing ring_;                  // the minibatch objects the fused and the sharded loop rotate (batch_ring.h)
  SGDDataCache cache_;             // data_cache = hbm: the row buffers of the parts read so far; destroyed with the learner
  FILE* pred_file_ = nullptr;       // open while a prediction job runs
  std::vector<float> pred_buf_;
  dfh_eval* eval_ = nullptr;        // exact_metrics = 1: the rows of the current validation / prediction pass
  // pred_write = device: the open unit's predictions, two text buffers (unit u is written while unit u + 1 is stepped and
  // downloaded), the write under way, and the job's counts for its log line
  dfh_predtext* predtext_ = nullptr;
  std::vector<char> pred_text_[2];
  int pred_text_cur_ = 0;
  std::future<void> pred_write_;
  size_t pred_unit_n_ = 0;
  struct PredCounts { size_t dev_rows = 0, dev_units = 0, host_rows = 0, host_units = 0; } pred_counts_;
};

}  // namespace difacto
#endif  // DIFACTO_HOST_SGD_LEARNER_H_
