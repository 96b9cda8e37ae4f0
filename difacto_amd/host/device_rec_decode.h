/**
 * device_rec_decode.h — rec_decode = device: the ParseHook that hands the records of a .rec file to the device
 * (dfh_textchunk_decode_crb: the compressed record is uploaded and its LZ4 blocks decoded there, 8 B per row come back), shared
 * by the SGD learner's device feed and by task = convert.  Built like DeviceTextParse: a regular record (ids only: no values, no
 * weights, as criteo records are) keeps its ids in HBM with the chunk's container (RowChunk::dev, a dfh_textchunk that travels
 * through the reader's pool); any other record is left to DecompressRowBlock on the parser thread — with its CHECKs and their
 * messages — and counted.
 */
#ifndef DIFACTO_HOST_DEVICE_REC_DECODE_H_
#define DIFACTO_HOST_DEVICE_REC_DECODE_H_
#include <algorithm>
#include <atomic>
#include <memory>
#include <string>
#include <vector>
#include "./batch_reader.h"
#include "./device_context.h"
#include "./device_text_parse.h"

namespace difacto {

struct DeviceRecDecode {
  // parser threads of a reader whose records the device decodes: a thread uploads a record and waits for the device twice,
  // so a few keep the copy of one record beside the kernels of another (DeviceTextParse::kThreads, for the same reason)
  static constexpr int kThreads = DeviceTextParse::kThreads;
  std::atomic<size_t> records{0}, fallback{0};

  /*! \brief the hook; *this outlives the reader it is installed in */
  ParseHook Hook(dfh_ctx* ctx) {
    return [this, ctx](const RawChunk& raw, RowChunk* out) {
      if (!out->dev) {   // (the container comes out of the reader's pool: its device-side arrays are reused like its vectors)
        dfh_textchunk* tc = nullptr;
        DFH_CALL(dfh_textchunk_create(ctx, 1, &tc));
        out->dev = std::shared_ptr<void>(tc, [](void* p) { dfh_textchunk_destroy(static_cast<dfh_textchunk*>(p)); });
      }
      dfh_textchunk* tc = static_cast<dfh_textchunk*>(out->dev.get());
      int regular = 0;
      size_t nrows = 0, nnz = 0;
      DFH_CALL(dfh_textchunk_decode_crb(tc, raw.data, raw.size, &regular, &nrows, &nnz));
      ++records;
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

  /*! \brief the job's line: how many records of `uri` the device decoded */
  void Log(const std::string& uri) const {
    const size_t nf = fallback.load(), nr = records.load();
    LOG(INFO) << "rec_decode=device: " << nr - nf << " of " << nr << " records of " << uri << " decoded on the device, " << nf
              << " fell back to the host decoder";
    if (nf) LOG(WARNING) << "rec_decode=device: " << nf << " of " << nr << " records carry values or weights, or are not what the "
                            "device decoder takes, and were inflated on the host";
  }
};

}  // namespace difacto
#endif  // DIFACTO_HOST_DEVICE_REC_DECODE_H_
