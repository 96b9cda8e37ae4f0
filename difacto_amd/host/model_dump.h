/**
 * model_dump.h — task = dump: model_in (a model file, or the parts its manifest names; learner = sgd, lbfgs and bcd write the
 * same format) as text in dump_out, one line "<id>\t<w>[\t<V_0> .. \t<V_{k-1}>]\n" per entry with w != 0 or V, in ascending
 * order of the printed id, every float as %.9g (which round-trips a float: the text loses nothing).  Learner-independent, like
 * Converter.  The parts are loaded into one table in HBM; the device selects and sorts the entries once and formats them a
 * UNIT of dump_unit_rows entries at a time (csrc/dfh_dumptext.hip through dfh_dump_*).  A unit with a value the device does not
 * format (non-finite, subnormal, |v| < 2^-64, |v| >= 2^32) is written by the host's fprintf from dfh_dump_entries, so the file
 * is exact on any model; dump_write = host takes that path for every unit (the yardstick, and the way out).  The host holds
 * two units at a time: one on its way to the file on a thread of its own while the next is formatted.
 */
#ifndef DIFACTO_HOST_MODEL_DUMP_H_
#define DIFACTO_HOST_MODEL_DUMP_H_
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <future>
#include <string>
#include <vector>
#include "./device_context.h"
#include "./model_parts.h"
#include "dmlc/parameter.h"

namespace difacto {

struct ModelDumpParam : public dmlc::Parameter<ModelDumpParam> {
  /** \brief the model: a file, or the name whose <model_in>.parts manifest names the parts of a sharded save */
  std::string model_in;
  /** \brief the text file to write (under <dump_out>.tmp until it is complete) */
  std::string dump_out;
  /** \brief feature (default): ids as they stand in the data file, ReverseBytes of the stored key; key: the stored keys */
  std::string dump_ids;
  /** \brief device (default) | host: where a unit's text is formatted */
  std::string dump_write;
  /** \brief entries per unit: one format call, one download, one write */
  int dump_unit_rows;
  DMLC_DECLARE_PARAMETER(ModelDumpParam) {
    DMLC_DECLARE_FIELD(model_in).set_default("");
    DMLC_DECLARE_FIELD(dump_out).set_default("");
    DMLC_DECLARE_FIELD(dump_ids).set_default("feature");
    DMLC_DECLARE_FIELD(dump_write).set_default("device");
    DMLC_DECLARE_FIELD(dump_unit_rows).set_default(65536);
  }
};

class ModelDump {
 public:
  /*! \brief everything that can be refused is refused here, before the device is touched */
  KWArgs Init(const KWArgs& kwargs) {
    auto remain = param_.InitAllowUnknown(kwargs);
    CHECK(getenv("DMLC_ROLE") == nullptr) << "task=dump in the environment of a rank (DMLC_ROLE is set): one process dumps a model, "
                                             "a sharded one through its manifest; run it without the ranks' environment";
    CHECK(!param_.model_in.empty()) << "task=dump needs model_in, the model file (or the name of a sharded model's manifest) to read";
    CHECK(!param_.dump_out.empty()) << "task=dump needs dump_out, the text file to write";
    CHECK(param_.dump_ids == "feature" || param_.dump_ids == "key")
        << "dump_ids=" << param_.dump_ids << " is not one of feature (the default: ids as in the data file) and key (the stored keys)";
    CHECK(param_.dump_write == "device" || param_.dump_write == "host")
        << "dump_write=" << param_.dump_write << " is not one of device (the default) and host";
    CHECK_GE(param_.dump_unit_rows, 1) << "dump_unit_rows=" << param_.dump_unit_rows << ": a unit has 1 entry or more";
    files_ = ModelInFiles(param_.model_in);   // fatal with the path when nothing is readable
    for (size_t i = 0; i < files_.size(); ++i) {
      int k = 0;
      uint64_t n = 0;
      ReadModelHeader(files_[i], &k, &n);
      CHECK(i == 0 || k == V_dim_) << files_[i] << " has V_dim = " << k << ", " << files_[0] << " has " << V_dim_;
      V_dim_ = k;
      total_ += n;
    }
    return remain;
  }

  void Run() {
    const double t0 = Now();
    dfh_updater_param up;
    dfh_updater_param_default(&up, V_dim_);
    const uint64_t cap = std::min<uint64_t>(std::max<uint64_t>(total_ + total_ / 2 + 1024, 1024), (1ull << 28) - 1);
    dfh_table* t = nullptr;
    DFH_CALL(dfh_table_create(DeviceContext::Get(), &up, cap, &t));
    for (const auto& path : files_) DFH_CALL(dfh_table_load(t, path.c_str(), 0, 0, nullptr, nullptr));
    LOG(INFO) << "loaded " << total_ << " entries of V_dim " << V_dim_ << " from " << files_.size() << (files_.size() == 1 ? " file" : " files")
              << " (" << dfh_table_bytes(t) << " bytes in HBM)";
    const double t1 = Now();
    dfh_dump* d = nullptr;
    uint64_t n = 0, n_with_V = 0;
    DFH_CALL(dfh_dump_open(t, param_.dump_ids == "feature" ? DFH_DUMP_IDS_FEATURE : DFH_DUMP_IDS_KEY, &d, &n));
    DFH_CALL(dfh_dump_shape(d, nullptr, &n_with_V, nullptr));
    const bool device = param_.dump_write == "device" && dfh_dump_tile(d) > 0;
    if (param_.dump_write == "device" && !device)
      LOG(INFO) << "V_dim " << V_dim_ << ": a line does not fit the device formatter, every unit is formatted on the host";
    const std::string tmp = param_.dump_out + ".tmp";
    FILE* f = fopen(tmp.c_str(), "wb");
    CHECK(f != nullptr) << "cannot open " << tmp << " for writing";
    std::vector<char> iobuf(1 << 22);
    setvbuf(f, iobuf.data(), _IOFBF, iobuf.size());
    const size_t unit = static_cast<size_t>(param_.dump_unit_rows);
    std::future<void> write;   // unit u - 1 on its way to the file, out of the other buffer
    int cur = 0;
    for (uint64_t at = 0; at < n; at += unit, cur ^= 1) {
      Unit* u = &unit_[cur];
      u->count = static_cast<size_t>(std::min<uint64_t>(unit, n - at));
      u->host = !device;
      if (device) {
        size_t nbytes = 0;
        uint64_t irregular = 0;
        DFH_CALL(dfh_dump_format(d, at, u->count, &nbytes, &irregular));
        u->host = irregular != 0;
        if (!u->host) {
          u->text.resize(nbytes);
          DFH_CALL(dfh_dump_read(d, u->text.data()));
        }
      }
      if (u->host) {
        u->ids.resize(u->count);
        u->w.resize(u->count);
        u->has_V.resize(u->count);
        u->V.resize(std::max<size_t>(u->count * static_cast<size_t>(V_dim_), 1));
        DFH_CALL(dfh_dump_entries(d, at, u->count, u->ids.data(), u->w.data(), u->has_V.data(), u->V.data()));
      }
      (u->host ? host_units_ : dev_units_) += 1;
      (u->host ? host_entries_ : dev_entries_) += u->count;
      if (write.valid()) write.get();
      const int k = V_dim_;
      const std::string* name = &tmp;
      write = std::async(std::launch::async, [u, f, k, name] { WriteUnit(*u, f, k, *name); });
    }
    if (write.valid()) write.get();
    const long bytes = ftell(f);
    CHECK_EQ(fclose(f), 0) << "closing " << tmp << " failed";
    CHECK_EQ(rename(tmp.c_str(), param_.dump_out.c_str()), 0) << "cannot move " << tmp << " to " << param_.dump_out;
    DFH_CALL(dfh_dump_close(d));
    DFH_CALL(dfh_table_destroy(t));
    const double t2 = Now();
    LOG(INFO) << "task=dump dump_write=" << param_.dump_write << ": " << n << " entries (" << n_with_V << " with V) to " << param_.dump_out << ", "
              << dev_units_ << " units / " << dev_entries_ << " entries formatted on the device, " << host_units_ << " units / " << host_entries_
              << " entries on the host, " << bytes << " bytes; model loaded in " << t1 - t0 << " s, dumped in " << t2 - t1 << " s ("
              << static_cast<double>(n) / std::max(t2 - t1, 1e-9) << " entries/s, " << static_cast<double>(bytes) / 1e6 / std::max(t2 - t1, 1e-9)
              << " MB/s)";
  }

 private:
  struct Unit {
    size_t count = 0;
    bool host = false;
    std::vector<char> text;       // the device's text
    std::vector<uint64_t> ids;    // or the entries, for the host's fprintf
    std::vector<float> w, V;
    std::vector<int> has_V;
  };
  static double Now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
  static void WriteUnit(const Unit& u, FILE* f, int k, const std::string& name) {
    if (!u.host) {
      CHECK_EQ(fwrite(u.text.data(), 1, u.text.size(), f), u.text.size()) << "cannot write " << name;
      return;
    }
    bool ok = true;
    for (size_t i = 0; i < u.count; ++i) {
      ok = ok && fprintf(f, "%llu", static_cast<unsigned long long>(u.ids[i])) > 0 && fprintf(f, "\t%.9g", u.w[i]) > 0;
      if (u.has_V[i])
        for (int j = 0; j < k; ++j) ok = ok && fprintf(f, "\t%.9g", u.V[i * static_cast<size_t>(k) + j]) > 0;
      ok = ok && fputc('\n', f) != EOF;
    }
    CHECK(ok) << "cannot write " << name;
  }

  ModelDumpParam param_;
  std::vector<std::string> files_;
  int V_dim_ = 0;
  uint64_t total_ = 0;
  Unit unit_[2];
  uint64_t dev_units_ = 0, dev_entries_ = 0, host_units_ = 0, host_entries_ = 0;
};

}  // namespace difacto
#endif  // DIFACTO_HOST_MODEL_DUMP_H_
