/**
 * lbfgs_learner.h — LBFGSLearner: the reference's full-batch L-BFGS learner (src/lbfgs/lbfgs_learner.{h,cc}) with the
 * training data, the model and the whole optimiser state resident in HBM (dfh_lbfgs, include/difacto_hip.h).
 *
 * The scheduler loop (RunScheduler: direction, Wolfe line search, stop criteria, epoch-end callbacks) follows
 * lbfgs_learner.cc:14-126 line by line.  The jobs it issues there to workers and servers are calls on one dfh_lbfgs
 * object here.  One process on one GPU, or one process per GPU (DMLC_ROLE=worker, DMLC_NUM_WORKER, DIFACTO_RANK and
 * DIFACTO_RENDEZVOUS all set; example/run_local_gpus.sh): then every process is a worker for part <rank> of <world> of
 * the data and the server of one key range of the model (dfh_lbfgs_create_sharded), and every scalar the scheduler
 * decides on is a sum over the ranks, so all ranks print the same lines and stop at the same epoch.  The (2m+1)^2 B-matrix algebra of the two-loop recursion stays on the host
 * (lbfgs_mini::Twoloop), the vectors never leave the device.
 *
 * Differences from the reference:
 *   - no tile store on disk (data_cache is accepted and unused) and no thread pool (num_threads is accepted and unused)
 *   - model_out is written (the reference declares it and never writes it): the final weights in the format of
 *     learner = sgd's model_out, without optimiser state, so that task = predict learner = sgd model_in = ... scores them
 *   - model_out of a sharded run is <model_out>.part-<rank> plus the <model_out>.parts manifest, as learner = sgd writes it
 *   - model_in is read (the reference declares it, lbfgs_param.h:58, and never reads it): a warm start from the w and V
 *     of a model file of any learner (optimiser state in the file is ignored; with V_dim > 0 the file's V_dim must be
 *     the job's), a file or the parts of a sharded save; a sharded rank reads its own key range.  The s / y history is
 *     not restored and load_epoch keeps its meaning: the first epoch of the loop
 *   - l1 (the reference declares it for LBFGSUpdater and comments it out, lbfgs_param.h:84-93): with l1 > 0 the objective
 *     gains l1 |w|_1 on w (V keeps V_l2) and the learner runs orthant-wise L-BFGS (OWL-QN, Andrew & Gao 2007; the rules
 *     and their fp32 order are stated in csrc/dfh_owlqn.hip): the direction comes from the pseudo-gradient and is kept
 *     only where it descends along it; every line-search trial starts from the epoch's w0 and is projected onto its
 *     orthant; a trial is accepted on sufficient decrease alone, F(w) <= F(w0) + c1 sum pg (w - w0) (c2 is unused, the
 *     log says so once); s is the real displacement w - w0; a pair with <s, y> <= 0 is dropped before the two-loop
 *     coefficients; training stops with "pseudo-gradient is zero" when <pg, p> == 0 and with "no coordinate moved" when
 *     the accepted step changed nothing.  l1 = 0, the default, changes no call and no log line
 *   - a multi-process environment that is not complete (see above) is refused with a message; so is task = predict for
 *     a caller of Learner::Create("lbfgs") (the command line scores a model through learner = sgd's prediction path itself)
 */
#ifndef DIFACTO_HOST_LBFGS_LEARNER_H_
#define DIFACTO_HOST_LBFGS_LEARNER_H_
#include <functional>
#include <memory>
#include <string>
#include <vector>
#include "./comm_setup.h"
#include "./lbfgs_mini.h"
#include "./lbfgs_param.h"
#include "difacto/learner.h"
#include "difacto/sarray.h"
#include "difacto_hip.h"

namespace difacto {
namespace lbfgs {

/*! \brief lbfgs_utils.h:46-60 */
struct Progress {
  real_t objv;     // objective value on training data
  real_t auc;      // auc on training data
  real_t val_auc;  // auc on validation data
  real_t nnz_w;    // number of nonzero entries in the model
};

}  // namespace lbfgs

/*! \brief what the reference's LBFGSUpdater exposes to a learner's user (lbfgs_updater.h:12-33): its parameters and the
 * weight initializer; the state itself lives in the dfh_lbfgs object */
class LBFGSUpdater {
 public:
  KWArgs Init(const KWArgs& kwargs) { return param_.InitAllowUnknown(kwargs); }
  const LBFGSUpdaterParam& param() const { return param_; }
  typedef std::function<void(const SArray<int>& weight_lens, SArray<real_t>* weights)> WeightInitializer;
  void SetWeightInitializer(const WeightInitializer& initer) { weight_initializer_ = initer; }
  const WeightInitializer& weight_initializer() const { return weight_initializer_; }

 private:
  LBFGSUpdaterParam param_;
  WeightInitializer weight_initializer_ = nullptr;
};

class LBFGSLearner : public Learner {
 public:
  LBFGSLearner() {}
  virtual ~LBFGSLearner();
  KWArgs Init(const KWArgs& kwargs) override;

  void AddEpochEndCallback(const std::function<void(int epoch, const lbfgs::Progress& prog)>& callback) {
    epoch_end_callback_.push_back(callback);
  }
  LBFGSUpdater* GetUpdater() { return &updater_; }

 protected:
  void RunScheduler() override;
  void Process(const std::string& args, std::string* rets) override {}

 private:
  /*! \brief PrepareData (lbfgs_learner.cc:165-210): read the data into chunks resident on the device; returns
   * {ntrain, train chunks, train nnz, nval, val chunks, val nnz} */
  void PrepareData(std::vector<real_t>* rets);
  /*! \brief InitWeight (lbfgs_updater.h:33-76) with the weight initializer; returns {r(w), number of parameters} */
  void InitServer(std::vector<real_t>* rets);
  /*! \brief the epoch's search direction, written into the s history; returns <p, g> */
  float Direction();
  /*! \brief the Wolfe line search from objective objv along p (<p, g> = pg), starting at step; returns the accepted
   * objective, *auc = AUC x n of the last gradient pass */
  real_t LineSearch(real_t step, real_t objv, float pg, float* auc);
  /*! \brief model_in: warm start from a model file (dfh_lbfgs_set_model), after InitWeight and the weight initializer */
  void LoadModel(uint64_t nkeys);
  void SaveModel();

  LBFGSLearnerParam param_;
  LBFGSUpdater updater_;
  int nthreads_ = 1;
  dfh_lbfgs* obj_ = nullptr;
  // the sharded mode: this process is rank rank_ of world_; comm_ is NULL in one process
  int rank_ = 0, world_ = 1;
  dfh_comm* comm_ = nullptr;
  std::unique_ptr<FileExchange> files_;
  lbfgs_mini::Twoloop twoloop_;
  std::vector<std::function<void(int epoch, const lbfgs::Progress& prog)>> epoch_end_callback_;
};

}  // namespace difacto
#endif  // DIFACTO_HOST_LBFGS_LEARNER_H_
