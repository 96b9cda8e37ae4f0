/**
 * converter.h — task = convert (src/reader/converter.h): reads data_in chunk by chunk and writes it as libsvm text or as a
 * .rec file, one RecordIO record of one CompressedRowBlock per chunk.  The row blocks are compressed ON THE DEVICE
 * (csrc/dfh_lz4enc.hip through dfh_crb_*: the product carries no liblz4 and there is no host encoder); with text_parse = device
 * the chunks of a criteo file are parsed there too and their ids never leave HBM between the parse and the encoder.
 * shuffle_rows / val_fraction: the rows of the whole input are first collected in one row store in HBM (csrc/dfh_rowstore.hip),
 * ordered there, and the records of data_out and data_val_out are gathered out of that order (WriteOrdered).
 */
#ifndef DIFACTO_HOST_CONVERTER_H_
#define DIFACTO_HOST_CONVERTER_H_
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <future>
#include <memory>
#include <sstream>
#include <string>
#include <vector>
#include "./batch_reader.h"
#include "./device_context.h"
#include "./device_rec_decode.h"
#include "./device_text_parse.h"
#include "./recordio_writer.h"
#include "dmlc/parameter.h"

namespace difacto {

struct ConverterParam : public dmlc::Parameter<ConverterParam> {
  /** \brief the input file */
  std::string data_in;
  /** \brief the input format: libsvm, rec, criteo, criteo_test, adfea */
  std::string data_format;
  /** \brief the output file, or the prefix of the parts (part_size) */
  std::string data_out;
  /** \brief the output format: libsvm or rec */
  std::string data_out_format;
  /**
   * \brief MB of text input per chunk = per record of a .rec output.  16, not the reference's 512: a record is the unit the
   * .rec reader of this build hands to a parser thread and splits data parts at, and records of 512 MB would serialise the
   * read (and come close to what one LZ4 block holds).  DIFACTO_CHUNK_BYTES overrides, as in Reader
   */
  real_t chunk_size;
  /** \brief split the output into parts "<data_out>-part_<i>", a new one once a part holds part_size MB; -1: one file */
  int part_size;
  /** \brief host (default) | device: where criteo text is parsed */
  std::string text_parse;
  /** \brief host (default) | device: where the records of a data_format = rec input are inflated.  Without shuffle_rows / val_fraction the output has one record per input
   *  record; through the row store the rows are re-cut into records of equal size */
  std::string rec_decode;
  /** \brief 1: the rows of the whole input are written in a shuffled order (dfh_rowstore_order); 0 (default): in file order */
  int shuffle_rows;
  /** \brief the seed of that order */
  uint64_t shuffle_seed;
  /** \brief the last floor(val_fraction * n) rows of the order go to data_val_out instead of data_out; in [0, 1), default 0 */
  double val_fraction;
  /** \brief the validation output, in data_out_format; always one file */
  std::string data_val_out;
  DMLC_DECLARE_PARAMETER(ConverterParam) {
    DMLC_DECLARE_FIELD(shuffle_rows).set_default(0);
    DMLC_DECLARE_FIELD(shuffle_seed).set_default(0);
    DMLC_DECLARE_FIELD(val_fraction).set_default(0);
    DMLC_DECLARE_FIELD(data_val_out).set_default("");
    DMLC_DECLARE_FIELD(data_in).set_default("");
    DMLC_DECLARE_FIELD(data_format).set_default("libsvm");
    DMLC_DECLARE_FIELD(data_out).set_default("");
    DMLC_DECLARE_FIELD(data_out_format).set_default("");
    DMLC_DECLARE_FIELD(part_size).set_default(-1);
    DMLC_DECLARE_FIELD(chunk_size).set_default(16);
    DMLC_DECLARE_FIELD(text_parse).set_default("host");
    DMLC_DECLARE_FIELD(rec_decode).set_default("host");
  }
};

class Converter {
 public:
  /*! \brief everything that can be refused is refused here, before the device is touched */
  KWArgs Init(const KWArgs& kwargs) {
    auto remain = param_.InitAllowUnknown(kwargs);
    CHECK(getenv("DMLC_ROLE") == nullptr) << "task=convert in the environment of a rank (DMLC_ROLE is set): a conversion is one "
                                             "process that reads the whole input; run it without the ranks' environment";
    CHECK(!param_.data_in.empty()) << "task=convert needs data_in, the file to read";
    CHECK(!param_.data_out.empty()) << "task=convert needs data_out, the file (or, with part_size, the prefix) to write";
    CHECK(param_.data_out_format == "libsvm" || param_.data_out_format == "rec")
        << "data_out_format=" << param_.data_out_format << ": task=convert writes libsvm or rec";
    CHECK(param_.text_parse == "host" || param_.text_parse == "device")
        << "text_parse=" << param_.text_parse << " is not one of host (the default) and device";
    CHECK(param_.text_parse != "device" || param_.data_format == "criteo" || param_.data_format == "criteo_test")
        << "text_parse=device with data_format=" << param_.data_format << ": the device parses criteo and criteo_test text only";
    CHECK(param_.rec_decode == "host" || param_.rec_decode == "device")
        << "rec_decode=" << param_.rec_decode << " is not one of host (the default) and device";
    CHECK(param_.rec_decode != "device" || param_.data_format == "rec")
        << "rec_decode=device with data_format=" << param_.data_format << ": the device decodes the records of rec files only";
    CHECK_GT(param_.chunk_size, 0) << "chunk_size is a size in MB";
    CHECK(param_.shuffle_rows == 0 || param_.shuffle_rows == 1)
        << "shuffle_rows=" << param_.shuffle_rows << " is not one of 0 (file order, the default) and 1";
    CHECK(param_.val_fraction >= 0 && param_.val_fraction < 1)
        << "val_fraction=" << param_.val_fraction << ": the share of the rows that goes to data_val_out lies in [0, 1)";
    CHECK(!(param_.val_fraction > 0) || !param_.data_val_out.empty())
        << "val_fraction=" << param_.val_fraction << " needs data_val_out, the file the validation rows are written to";
    CHECK(param_.val_fraction > 0 || param_.data_val_out.empty())
        << "data_val_out=" << param_.data_val_out << " with val_fraction=0: no row would be written to it; give val_fraction";
    CHECK(param_.data_val_out.empty() || param_.data_val_out != param_.data_out)
        << "data_val_out and data_out are the same file, " << param_.data_out;
    return remain;
  }

  void Run() {
    dfh_ctx* ctx = DeviceContext::Get();   // (created once, like in every run of the command line)
    const bool rec = param_.data_out_format == "rec";
    const bool device_parse = param_.text_parse == "device";
    DeviceTextParse text_parse;   // outlives the reader
    ParseHook hook;
    if (device_parse && rec) hook = text_parse.Hook(ctx, param_.data_format == "criteo" ? 1 : 0);
    DeviceRecDecode rec_decode;   // the same for the records of a .rec input
    const bool device_decode = param_.rec_decode == "device" && rec;
    if (device_decode) hook = rec_decode.Hook(ctx);
    const size_t chunk_bytes = static_cast<size_t>(static_cast<double>(param_.chunk_size) * 1024 * 1024);
    const int threads = !hook || getenv("DIFACTO_PARSER_THREADS") != nullptr ? 0 : (device_decode ? DeviceRecDecode::kThreads : DeviceTextParse::kThreads);
    Reader in(param_.data_in, param_.data_format, 0, 1, std::max<size_t>(chunk_bytes, 64), threads, hook);
    LOG(INFO) << "reading data from " << param_.data_in << " in " << param_.data_format << " format";
    // a small pool of encoders: the encode of chunk t + 1 runs while the record of chunk t is copied back and written
    std::vector<dfh_crb*> pool(rec ? kEncoders : 0, nullptr);
    for (auto& e : pool) DFH_CALL(dfh_crb_create(ctx, &e));
    out_name_ = param_.data_out;
    parts_ = param_.part_size >= 0;
    if (param_.shuffle_rows || param_.val_fraction > 0) {
      WriteOrdered(ctx, &in, pool);
      for (auto e : pool) dfh_crb_destroy(e);
      Close();
      LOG(INFO) << "done. written " << nwrite_ << " bytes";
      if (device_parse && hook) text_parse.Log(param_.data_in);
      if (device_decode) rec_decode.Log(param_.data_in);
      return;
    }
    std::deque<std::future<Encoded>> pending;   // in file order
    size_t taken = 0;
    std::shared_ptr<RowChunk> chunk;
    while (in.NextShared(&chunk)) {
      if (!rec) {
        WriteLibsvm(ViewOf(*chunk));
        continue;
      }
      if (pending.size() == pool.size()) {   // the oldest encode is the one whose encoder comes free
        WriteRecord(pending.front().get());
        pending.pop_front();
      }
      dfh_crb* e = pool[taken++ % pool.size()];
      pending.push_back(std::async(std::launch::async, [e, chunk] { return Encode(e, *chunk); }));
      chunk.reset();
    }
    for (; !pending.empty(); pending.pop_front()) WriteRecord(pending.front().get());
    for (auto e : pool) dfh_crb_destroy(e);
    Close();
    LOG(INFO) << "done. written " << nwrite_ << " bytes";
    if (device_parse && hook) text_parse.Log(param_.data_in);
    if (device_decode) rec_decode.Log(param_.data_in);
  }

 private:
  static const int kEncoders = 3;
  struct Encoded {
    size_t nrows = 0;
    std::string record;
  };
  static Encoded Encode(dfh_crb* e, const RowChunk& c) {
    Encoded out;
    out.nrows = c.offset.size() - 1;
    size_t bytes = 0;
    if (c.on_device) {
      DFH_CALL(dfh_crb_encode_textchunk(e, static_cast<dfh_textchunk*>(c.dev.get()), &bytes));
    } else {
      const size_t first = c.offset[0];
      DFH_CALL(dfh_crb_encode_host(e, out.nrows, c.offset.data(), c.label.data(), c.index.empty() ? nullptr : c.index.data() + first,
                                   c.value.empty() ? nullptr : c.value.data() + first, c.weight.empty() ? nullptr : c.weight.data(),
                                   &bytes));
    }
    out.record.resize(bytes);
    DFH_CALL(dfh_crb_record(e, &out.record[0]));
    return out;
  }
  static Encoded EncodeRows(dfh_crb* e, dfh_rowstore* st, uint64_t first, size_t count) {
    Encoded out;
    out.nrows = count;
    size_t bytes = 0;
    DFH_CALL(dfh_crb_encode_rowstore(e, st, first, count, &bytes));
    out.record.resize(bytes);
    DFH_CALL(dfh_crb_record(e, &out.record[0]));
    return out;
  }
  /*!
   * \brief shuffle_rows / val_fraction: every chunk is appended to one row store in HBM, in file order (a regular device-parsed
   * chunk device to device); at the end of the input the order is fixed once, and the outputs are cut out of it in records of
   * R = ceil(n / C) rows, C the input's non-empty chunks — the record size of an unshuffled conversion.  Nothing can be written
   * before the last chunk is in.  An input that does not fit in HBM ends the run with the store's capacity message
   */
  void WriteOrdered(dfh_ctx* ctx, Reader* in, const std::vector<dfh_crb*>& pool) {
    dfh_rowstore* st = nullptr;
    const char* slab = getenv("DIFACTO_SLAB_BYTES");   // (tests: many slabs out of a small input)
    DFH_CALL(dfh_rowstore_create(ctx, slab ? static_cast<size_t>(atoll(slab)) : 0, &st));
    std::shared_ptr<void> owner(st, [](void* p) { dfh_rowstore_destroy(static_cast<dfh_rowstore*>(p)); });
    uint64_t chunks = 0;
    std::shared_ptr<RowChunk> chunk;
    while (in->NextShared(&chunk)) {
      const RowChunk& c = *chunk;
      const size_t nrows = c.offset.size() - 1;
      if (nrows == 0) continue;
      ++chunks;
      if (c.on_device) {
        DFH_CALL(dfh_rowstore_append_textchunk(st, static_cast<dfh_textchunk*>(c.dev.get())));
      } else {
        const size_t first = c.offset[0];
        DFH_CALL(dfh_rowstore_append_host(st, nrows, c.offset.data(), c.label.data(), c.index.empty() ? nullptr : c.index.data() + first,
                                          c.value.empty() ? nullptr : c.value.data() + first, c.weight.empty() ? nullptr : c.weight.data()));
      }
      chunk.reset();
    }
    DFH_CALL(dfh_rowstore_order(st, param_.shuffle_rows, param_.shuffle_seed));
    uint64_t n = 0, nnz = 0, device_bytes = 0;
    int has_value = 0, has_weight = 0;
    DFH_CALL(dfh_rowstore_shape(st, &n, &nnz, &has_value, &has_weight, &device_bytes));
    const uint64_t n_val = static_cast<uint64_t>(std::floor(param_.val_fraction * static_cast<double>(n)));
    const uint64_t R = std::max<uint64_t>(chunks ? (n + chunks - 1) / chunks : 1, 1);
    LOG(INFO) << "ordered " << n << " rows in HBM (" << device_bytes << " bytes): " << n - n_val << " training and " << n_val
              << " validation rows, records of " << R << " rows, shuffle_rows=" << param_.shuffle_rows << " shuffle_seed=" << param_.shuffle_seed;
    WriteRows(st, pool, 0, n - n_val, R, has_value != 0, has_weight != 0);
    if (param_.data_val_out.empty()) return;
    Close();
    LOG(INFO) << "done. written " << nwrite_ << " bytes";
    out_name_ = param_.data_val_out;
    parts_ = false;
    nwrite_ = nrows_ = 0;
    WriteRows(st, pool, n - n_val, n_val, R, has_value != 0, has_weight != 0);
  }
  /*! \brief rows order[first .. first + count) to the current output, R per record (per piece of libsvm text) */
  void WriteRows(dfh_rowstore* st, const std::vector<dfh_crb*>& pool, uint64_t first, uint64_t count, uint64_t R, bool has_value,
                 bool has_weight) {
    if (count == 0) NextFile();   // (the file exists even when no row goes to it)
    if (pool.empty()) {
      std::vector<size_t> offset;
      std::vector<real_t> label, value, weight;
      std::vector<feaid_t> index;
      for (uint64_t at = first; at < first + count; at += R) {
        const size_t cnt = static_cast<size_t>(std::min<uint64_t>(R, first + count - at));
        size_t nnz = 0;
        offset.resize(cnt + 1);
        label.resize(cnt);
        DFH_CALL(dfh_rowstore_read(st, at, cnt, offset.data(), label.data(), nullptr, nullptr, nullptr, &nnz));
        index.resize(std::max<size_t>(nnz, 1));
        if (has_value) value.resize(std::max<size_t>(nnz, 1));
        if (has_weight) weight.resize(cnt);
        DFH_CALL(dfh_rowstore_read(st, at, cnt, offset.data(), label.data(), index.data(), has_value ? value.data() : nullptr,
                                   has_weight ? weight.data() : nullptr, &nnz));
        dmlc::RowBlock<feaid_t> blk;
        blk.size = cnt;
        blk.offset = offset.data();
        blk.label = label.data();
        blk.weight = has_weight ? weight.data() : nullptr;
        blk.index = index.data();
        blk.value = has_value ? value.data() : nullptr;
        WriteLibsvm(blk);
      }
      return;
    }
    std::deque<std::future<Encoded>> pending;   // in the order's order
    size_t taken = 0;
    for (uint64_t at = first; at < first + count; at += R) {
      const size_t cnt = static_cast<size_t>(std::min<uint64_t>(R, first + count - at));
      if (pending.size() == pool.size()) {
        WriteRecord(pending.front().get());
        pending.pop_front();
      }
      dfh_crb* e = pool[taken++ % pool.size()];
      pending.push_back(std::async(std::launch::async, [e, st, at, cnt] { return EncodeRows(e, st, at, cnt); }));
    }
    for (; !pending.empty(); pending.pop_front()) WriteRecord(pending.front().get());
  }
  /*! \brief a new part when there is no file yet, or the current one holds part_size MB (converter.h:68-79) */
  void NextFile() {
    const bool parts = parts_;
    if (out_ && !(parts && nwrite_ / 1000000 >= static_cast<size_t>(param_.part_size))) return;
    if (out_) LOG(INFO) << "done. written " << nwrite_ << " bytes";
    Close();
    const std::string name = parts ? out_name_ + "-part_" + std::to_string(ipart_++) : out_name_;
    out_ = fopen(name.c_str(), "wb");
    CHECK(out_ != nullptr) << "cannot open " << name << " for writing";
    nwrite_ = 0;
    LOG(INFO) << "writing data to " << name << " in " << param_.data_out_format << " format";
  }
  void Close() {
    if (out_) CHECK_EQ(fclose(out_), 0) << "closing the output failed";
    out_ = nullptr;
  }
  void Put(const std::string& bytes) {
    CHECK_EQ(fwrite(bytes.data(), 1, bytes.size(), out_), bytes.size()) << "writing the output failed";
  }
  void WriteRecord(const Encoded& enc) {
    NextFile();
    framed_.clear();
    RecordIOWriter::Append(enc.record.data(), enc.record.size(), &framed_);
    Put(framed_);
    nwrite_ += enc.record.size();   // the payloads, as the reference counts (converter.h:108)
    nrows_ += enc.nrows;
    LOG(INFO) << "written " << nrows_ << " examples in " << nwrite_ << " bytes";
  }
  /*! \brief converter.h:91-101: label, then index[:value] separated by blanks, the stream's default number formatting */
  void WriteLibsvm(const dmlc::RowBlock<feaid_t>& blk) {
    NextFile();
    std::ostringstream os;
    for (size_t i = 0; i < blk.size; ++i) {
      os << blk.label[i] << " ";
      for (size_t j = blk.offset[i]; j < blk.offset[i + 1]; ++j) {
        os << blk.index[j];
        if (blk.value) os << ":" << blk.value[j];
        os << " ";
      }
      os << "\n";
    }
    const std::string text = os.str();
    Put(text);
    nwrite_ += text.size();
    nrows_ += blk.size;
    LOG(INFO) << "written " << nrows_ << " examples in " << nwrite_ << " bytes";
  }

  ConverterParam param_;
  FILE* out_ = nullptr;
  std::string out_name_;   // the output being written: data_out (or the prefix of its parts), then data_val_out
  bool parts_ = false;
  int ipart_ = 0;
  size_t nwrite_ = 0, nrows_ = 0;
  std::string framed_;
};

}  // namespace difacto
#endif  // DIFACTO_HOST_CONVERTER_H_
