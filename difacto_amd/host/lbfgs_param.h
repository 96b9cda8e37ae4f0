/**
 * lbfgs_param.h — the L-BFGS learner's parameters: the same keys, defaults and ranges as the reference
 * (src/lbfgs/lbfgs_param.h:9-99).  data_cache and num_threads are accepted and have no effect here (the data stay
 * resident in HBM, the work runs on the GPU).  One key more than the reference reads: l1, which its LBFGSUpdaterParam
 * declares and comments out (:84-93).  Here l1 > 0 trains w by orthant-wise L-BFGS (lbfgs_learner.h); l1 = 0, the
 * default, is the reference's learner.
 */
#ifndef DIFACTO_HOST_LBFGS_PARAM_H_
#define DIFACTO_HOST_LBFGS_PARAM_H_
#include <string>
#include "difacto/base.h"
#include "dmlc/parameter.h"

namespace difacto {

struct LBFGSLearnerParam : public dmlc::Parameter<LBFGSLearnerParam> {
  std::string data_in, data_val, data_format, data_cache, model_out, model_in, loss;
  int max_num_epochs, min_num_epochs;
  real_t data_chunk_size;   // MB of input per chunk
  real_t stop_rel_objv, stop_val_auc;
  int load_epoch;
  real_t init_alpha, alpha, c1, c2, rho, gamma;
  int max_num_linesearchs;
  int num_threads;
  DMLC_DECLARE_PARAMETER(LBFGSLearnerParam) {
    DMLC_DECLARE_FIELD(data_in);
    DMLC_DECLARE_FIELD(data_val).set_default("");
    DMLC_DECLARE_FIELD(data_format).set_default("libsvm");
    DMLC_DECLARE_FIELD(data_cache).set_default("/tmp/difacto_lbfgs_");
    DMLC_DECLARE_FIELD(data_chunk_size).set_default(256);
    DMLC_DECLARE_FIELD(model_out).set_default("");
    DMLC_DECLARE_FIELD(model_in).set_default("");
    DMLC_DECLARE_FIELD(loss).set_default("fm");
    DMLC_DECLARE_FIELD(max_num_epochs).set_default(100);
    DMLC_DECLARE_FIELD(min_num_epochs).set_default(10);
    DMLC_DECLARE_FIELD(alpha).set_default(1);
    DMLC_DECLARE_FIELD(init_alpha).set_default(0);
    DMLC_DECLARE_FIELD(max_num_linesearchs).set_default(5);
    DMLC_DECLARE_FIELD(c1).set_default(1e-4);
    DMLC_DECLARE_FIELD(gamma).set_default(1);
    DMLC_DECLARE_FIELD(c2).set_default(.9);
    DMLC_DECLARE_FIELD(rho).set_default(.5);
    DMLC_DECLARE_FIELD(load_epoch).set_default(0);
    DMLC_DECLARE_FIELD(stop_rel_objv).set_default(1e-5);
    DMLC_DECLARE_FIELD(stop_val_auc).set_default(1e-5);
    DMLC_DECLARE_FIELD(num_threads).set_default(0);
  }
};

struct LBFGSUpdaterParam : public dmlc::Parameter<LBFGSUpdaterParam> {
  int V_dim;
  int V_threshold;
  float V_init_scale;
  int tail_feature_filter;
  float l1, l2, V_l2;
  int m;
  DMLC_DECLARE_PARAMETER(LBFGSUpdaterParam) {
    DMLC_DECLARE_FIELD(tail_feature_filter).set_default(4);
    DMLC_DECLARE_FIELD(l1).set_range(0, 1e10).set_default(0);
    DMLC_DECLARE_FIELD(l2).set_default(.1);
    DMLC_DECLARE_FIELD(V_l2).set_default(.01);
    DMLC_DECLARE_FIELD(V_dim);
    DMLC_DECLARE_FIELD(V_threshold).set_default(0);
    DMLC_DECLARE_FIELD(m).set_default(10);
    DMLC_DECLARE_FIELD(V_init_scale).set_default(.01);
  }
};

}  // namespace difacto
#endif  // DIFACTO_HOST_LBFGS_PARAM_H_
