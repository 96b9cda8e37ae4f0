/**
 * main.cc — the `difacto` command line: key=value arguments, `argfile=x.conf`
 * pulls in a config file (same "k = v" / '#' comment format as the reference's
 * example/<name>.conf), `task=train learner=sgd` by default; unknown keys are
 * reported as warnings.  Reference: src/main.cc, src/common/arg_parser.h.
 */
#include <chrono>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include "./converter.h"
#include "./model_dump.h"
#include "difacto/learner.h"
#include "dmlc/config.h"
#include "dmlc/parameter.h"

namespace difacto {

struct DifactoParam : public dmlc::Parameter<DifactoParam> {
  std::string task;     // train (default) | predict | convert | dump
  std::string learner;  // sgd
  DMLC_DECLARE_PARAMETER(DifactoParam) {
    DMLC_DECLARE_FIELD(learner).set_default("sgd");
    DMLC_DECLARE_FIELD(task).set_default("train");
  }
};
DMLC_REGISTER_PARAMETER(DifactoParam);
DMLC_REGISTER_PARAMETER(ConverterParam);
DMLC_REGISTER_PARAMETER(ModelDumpParam);

/*! \brief collects argv tokens and config-file text, then parses them as one "k = v" stream */
class ArgParser {
 public:
  void AddArg(const char* argv) {
    data_.append(argv);
    data_.append(" ");
  }
  KWArgs GetKWArgs() {
    std::unique_ptr<dmlc::Config> conf = Parse();
    for (const auto& it : *conf) {
      if (it.first == "argfile") {
        std::ifstream in(it.second.c_str());
        CHECK(in.good()) << "failed to open " << it.second;
        std::stringstream ss;
        ss << in.rdbuf();
        data_.append(ss.str());
        data_.append(" ");
        conf = Parse();
        break;
      }
    }
    KWArgs kwargs;
    for (const auto& it : *conf)
      if (it.first != "argfile") kwargs.push_back(it);
    return kwargs;
  }

 private:
  std::unique_ptr<dmlc::Config> Parse() {
    std::stringstream ss(data_);
    return std::unique_ptr<dmlc::Config>(new dmlc::Config(ss));
  }
  std::string data_;
};

void WarnUnknownKWArgs(const DifactoParam& param, const KWArgs& remain) {
  if (remain.empty()) return;
  LOG(WARNING) << "Unrecognized keyword argument for task = " << param.task;
  for (const auto& kw : remain) LOG(WARNING) << " - " << kw.first << " = " << kw.second;
}

}  // namespace difacto

int main(int argc, char* argv[]) {
  if (argc < 2) {
    LOG(ERROR) << "usage: difacto key1=val1 key2=val2 ...";
    return 0;
  }
  using namespace difacto;
  // DIFACTO_PROFILE=1: where the PROCESS spends its wall-clock outside the worker loop (start-up and teardown are most of a
  // one-epoch job: profiles/r05e_e2e_startup.txt)
  const bool prof = getenv("DIFACTO_PROFILE") != nullptr;
  auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  const double t0 = now();
  ArgParser parser;
  for (int i = 1; i < argc; ++i) parser.AddArg(argv[i]);
  DifactoParam param;
  auto kwargs_remain = param.InitAllowUnknown(parser.GetKWArgs());
  // text_parse = device is a key of learner = sgd's device feed: the other learners would only warn about a key they do not know
  for (const auto& kw : kwargs_remain)
    CHECK(!(kw.first == "text_parse" && kw.second == "device" && param.learner != "sgd" && param.task != "convert"))
        << "text_parse=device with learner=" << param.learner << ": only learner=sgd reads its training data through the device "
           "feed, whose text the device parses; leave text_parse out";
  for (const auto& kw : kwargs_remain)
    CHECK(!(kw.first == "rec_decode" && kw.second == "device" && param.learner != "sgd" && param.task != "convert"))
        << "rec_decode=device with learner=" << param.learner << ": only learner=sgd reads its training data through the device "
           "feed, whose records the device decodes; leave rec_decode out";
  if (param.task == "train") {
    Learner* learner = Learner::Create(param.learner);
    WarnUnknownKWArgs(param, learner->Init(kwargs_remain));
    const double t1 = now();
    learner->Run();
    const double t2 = now();
    delete learner;
    if (prof)
      LOG(INFO) << "process: main() to the learner initialised (HIP runtime, device context, model table) " << t1 - t0 << " s, Run "
                << t2 - t1 << " s, learner destroyed in " << now() - t2 << " s";
  } else if (param.task == "predict") {
    // the reference stops at a TODO here (main.cc:61-62); its SGDLearnerParam already names model_in as the model of
    // "a prediction task" (sgd_param.h:24-28).  The learner runs one forward pass over the data and writes pred_out.
    // A prediction needs no training data and no learner state: a model_in of learner = lbfgs or bcd is scored by the SGD
    // learner's prediction path with the same remaining arguments (for bcd: V_dim = 0, its models carry no V).  Without
    // a model_in there is nothing to score: the learner's own Init refuses and says how a model is written and scored.
    std::string type = param.learner;
    bool has_model = false;
    for (const auto& kw : kwargs_remain) has_model = has_model || (kw.first == "model_in" && kw.second.size());
    if (has_model && (type == "lbfgs" || type == "bcd")) {
      if (type == "bcd") {
        bool given = false;
        for (const auto& kw : kwargs_remain) {
          if (kw.first != "V_dim") continue;
          CHECK_EQ(atoi(kw.second.c_str()), 0) << "task = predict learner = bcd scores a linear model: V_dim = " << kw.second
                                               << " is not 0";
          given = true;
        }
        if (!given) kwargs_remain.push_back(std::make_pair("V_dim", "0"));
      }
      type = "sgd";
    }
    Learner* learner = Learner::Create(type);
    kwargs_remain.push_back(std::make_pair("task", "predict"));
    WarnUnknownKWArgs(param, learner->Init(kwargs_remain));
    learner->Run();
    delete learner;
  } else if (param.task == "convert") {
    // src/main.cc:57-60: data_in -> data_out (libsvm or rec); the row blocks of a .rec file are compressed on the device
    Converter converter;
    WarnUnknownKWArgs(param, converter.Init(kwargs_remain));
    converter.Run();
  } else if (param.task == "dump") {
    // model_in -> dump_out: the model as sorted text, "<id>\t<w>[\t<V_j>]" per entry, formatted on the device
    ModelDump dump;
    WarnUnknownKWArgs(param, dump.Init(kwargs_remain));
    dump.Run();
  } else {
    LOG(FATAL) << "unknown task: " << param.task << " (this build provides train, predict, convert and dump)";
  }
  return 0;
}
