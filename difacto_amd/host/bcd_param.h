/**
 * bcd_param.h — the BCD learner's and updater's parameters: the same keys and defaults as the reference
 * (src/bcd/bcd_param.h:10-56, src/bcd/bcd_updater.h:20-37).  data_cache is accepted and has no effect here (the data stay
 * resident in HBM); loss is accepted and ignored (the loss is always logit_delta, bcd_learner.cc:31); random_block and
 * l2 are declared and never read, as in the reference.  shard_rows is this build's: 1 = one process per GPU, the rows
 * split by rank (bcd_learner.h).
 */
#ifndef DIFACTO_HOST_BCD_PARAM_H_
#define DIFACTO_HOST_BCD_PARAM_H_
#include <string>
#include "difacto/base.h"
#include "dmlc/parameter.h"

namespace difacto {

struct BCDLearnerParam : public dmlc::Parameter<BCDLearnerParam> {
  std::string data_in, data_val, data_format, data_cache, model_out, model_in, loss;
  int max_num_epochs;
  float block_ratio;
  int random_block;
  int num_feature_group_bits;
  int data_chunk_size;   // bytes of input per chunk
  int shard_rows;        // 1: this process is one rank of DMLC_NUM_WORKER, each with part rank of the rows on its GPU
  DMLC_DECLARE_PARAMETER(BCDLearnerParam) {
    DMLC_DECLARE_FIELD(data_format).set_default("libsvm");
    DMLC_DECLARE_FIELD(data_in);
    DMLC_DECLARE_FIELD(data_val).set_default("");
    DMLC_DECLARE_FIELD(data_cache).set_default("/tmp/difacto_bcd_");
    DMLC_DECLARE_FIELD(data_chunk_size).set_default(1 << 28);
    DMLC_DECLARE_FIELD(model_out).set_default("");
    DMLC_DECLARE_FIELD(model_in).set_default("");
    DMLC_DECLARE_FIELD(loss).set_default("fm");
    DMLC_DECLARE_FIELD(max_num_epochs).set_default(20);
    DMLC_DECLARE_FIELD(random_block).set_default(1);
    DMLC_DECLARE_FIELD(num_feature_group_bits).set_default(0);
    DMLC_DECLARE_FIELD(block_ratio).set_default(4);
    DMLC_DECLARE_FIELD(shard_rows).set_default(0);
  }
};

struct BCDUpdaterParam : public dmlc::Parameter<BCDUpdaterParam> {
  int tail_feature_filter;
  float l1, l2, lr;
  DMLC_DECLARE_PARAMETER(BCDUpdaterParam) {
    DMLC_DECLARE_FIELD(tail_feature_filter).set_default(4);
    DMLC_DECLARE_FIELD(l1).set_default(1);
    DMLC_DECLARE_FIELD(l2).set_default(.01);
    DMLC_DECLARE_FIELD(lr).set_default(.9);
  }
};

}  // namespace difacto
#endif  // DIFACTO_HOST_BCD_PARAM_H_
