/**
 * converter.h — task = convert (src/reader/converter.h): reads data_in chunk by chunk and writes it as libsvm text or as a
 * .rec file, one RecordIO record of one CompressedRowBlock per chunk.  The row blocks are compressed ON THE DEVICE
 * (csrc/dfh_lz4enc.hip through dfh_crb_*: the product carries no liblz4 and there is no host encoder); with text_parse = device
 * the chunks of a criteo file are parsed there too and their ids never leave HBM between the parse and the encoder.
 */
#ifndef DIFACTO_HOST_CONVERTER_H_
#define DIFACTO_HOST_CONVERTER_H_
#include <cstdio>
#include <deque>
#include <future>
#include <memory>
#include <sstream>
#include <string>
#include <vector>
#include "./batch_reader.h"
#include "./device_context.h"
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
  DMLC_DECLARE_PARAMETER(ConverterParam) {
    DMLC_DECLARE_FIELD(data_in).set_default("");
    DMLC_DECLARE_FIELD(data_format).set_default("libsvm");
    DMLC_DECLARE_FIELD(data_out).set_default("");
    DMLC_DECLARE_FIELD(data_out_format).set_default("");
    DMLC_DECLARE_FIELD(part_size).set_default(-1);
    DMLC_DECLARE_FIELD(chunk_size).set_default(16);
    DMLC_DECLARE_FIELD(text_parse).set_default("host");
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
    CHECK_GT(param_.chunk_size, 0) << "chunk_size is a size in MB";
    return remain;
  }

  void Run() {
    dfh_ctx* ctx = DeviceContext::Get();   // (created once, like in every run of the command line)
    const bool rec = param_.data_out_format == "rec";
    const bool device_parse = param_.text_parse == "device";
    DeviceTextParse text_parse;   // outlives the reader
    ParseHook hook;
    if (device_parse && rec) hook = text_parse.Hook(ctx, param_.data_format == "criteo" ? 1 : 0);
    const size_t chunk_bytes = static_cast<size_t>(static_cast<double>(param_.chunk_size) * 1024 * 1024);
    const int threads = hook && getenv("DIFACTO_PARSER_THREADS") == nullptr ? DeviceTextParse::kThreads : 0;
    Reader in(param_.data_in, param_.data_format, 0, 1, std::max<size_t>(chunk_bytes, 64), threads, hook);
    LOG(INFO) << "reading data from " << param_.data_in << " in " << param_.data_format << " format";
    // a small pool of encoders: the encode of chunk t + 1 runs while the record of chunk t is copied back and written
    std::vector<dfh_crb*> pool(rec ? kEncoders : 0, nullptr);
    for (auto& e : pool) DFH_CALL(dfh_crb_create(ctx, &e));
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
    if (hook) text_parse.Log(param_.data_in);
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
  /*! \brief a new part when there is no file yet, or the current one holds part_size MB (converter.h:68-79) */
  void NextFile() {
    const bool parts = param_.part_size >= 0;
    if (out_ && !(parts && nwrite_ / 1000000 >= static_cast<size_t>(param_.part_size))) return;
    if (out_) LOG(INFO) << "done. written " << nwrite_ << " bytes";
    Close();
    const std::string name = parts ? param_.data_out + "-part_" + std::to_string(ipart_++) : param_.data_out;
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
  int ipart_ = 0;
  size_t nwrite_ = 0, nrows_ = 0;
  std::string framed_;
};

}  // namespace difacto
#endif  // DIFACTO_HOST_CONVERTER_H_
