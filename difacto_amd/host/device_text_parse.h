/**
 * device_text_parse.h — text_parse = device: the ParseHook that hands the chunks of a criteo file to the device
 * (dfh_textchunk_parse_criteo: upload, parse, 8 B per row back), shared by the SGD learner's device feed and by task = convert.
 * A regular chunk keeps its ids in HBM with the chunk's container (RowChunk::dev, a dfh_textchunk that travels through the
 * reader's pool and is reused like the container's vectors); a chunk that is not regular is left to the host parser and counted.
 */
#ifndef DIFACTO_HOST_DEVICE_TEXT_PARSE_H_
#define DIFACTO_HOST_DEVICE_TEXT_PARSE_H_
#include <algorithm>
#include <atomic>
#include <memory>
#include <string>
#include <vector>
#include "./batch_reader.h"
#include "./device_context.h"

namespace difacto {

struct DeviceTextParse {
  // parser threads of a reader whose chunks the device parses: a thread uploads a chunk and waits for the device, so a few
  // keep the copy of one chunk beside the kernels of another
  static constexpr int kThreads = 3;
  std::atomic<size_t> chunks{0}, fallback{0};

  /*! \brief the hook; *this outlives the reader it is installed in.  is_train_format: data_format = criteo (1) / criteo_test (0) */
  ParseHook Hook(dfh_ctx* ctx, int is_train_format) {
    return [this, ctx, is_train_format](const RawChunk& raw, RowChunk* out) {
      if (!out->dev) {   // (the container comes out of the reader's pool: its device-side arrays are reused like its vectors)
        dfh_textchunk* tc = nullptr;
        DFH_CALL(dfh_textchunk_create(ctx, std::max<size_t>(raw.size, 1), &tc));
        out->dev = std::shared_ptr<void>(tc, [](void* p) { dfh_textchunk_destroy(static_cast<dfh_textchunk*>(p)); });
      }
      dfh_textchunk* tc = static_cast<dfh_textchunk*>(out->dev.get());
      int regular = 0;
      size_t nrows = 0, nnz = 0;
      DFH_CALL(dfh_textchunk_parse_criteo(tc, raw.data, raw.size, is_train_format, &regular, &nrows, &nnz));
      ++chunks;
      if (!regular) {
        ++fallback;
        return false;
      }
      static thread_local std::vector<uint32_t> off32;
      off32.resize(nrows + 1);
      out->Clear();
      out->label.resize(nrows);
      DFH_CALL(dfh_textchunk_rows(tc, off32.data(), out->label.data()));
      out->offset.assign(off32.begin(), off32.end());
      out->on_device = true;
      return true;
    };
  }

  /*! \brief the job's line: how many chunks of `uri` the device parsed */
  void Log(const std::string& uri) const {
    const size_t nf = fallback.load(), nc = chunks.load();
    LOG(INFO) << "text_parse=device: " << nc - nf << " of " << nc << " chunks of " << uri << " parsed on the device, " << nf
              << " fell back to the host parser";
    if (nf) LOG(WARNING) << "text_parse=device: " << nf << " of " << nc << " chunks are not made of regular rows alone (CRLF, blank lines, "
                            "odd labels or field lengths) and were parsed on the host";
  }
};

}  // namespace difacto
#endif  // DIFACTO_HOST_DEVICE_TEXT_PARSE_H_
