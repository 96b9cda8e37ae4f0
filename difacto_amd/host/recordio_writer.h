/**
 * recordio_writer.h — dmlc-core's RecordIOWriter::WriteRecord (include/dmlc/recordio.h), restated from the published format
 * that RecordIOPart (batch_reader.h) reads:
 *     [magic 0xced7230a][cflag << 29 | length][payload, zero-padded to 4 bytes]
 * A payload that holds the magic word at a 4-byte-aligned position is cut there into parts (cflag 1: first, 2: middle,
 * 3: last; 0: a whole record) and the word itself is dropped; the reader puts it back between the parts.  Words that start at
 * other positions, and the last len % 4 bytes, are not looked at.
 */
#ifndef DIFACTO_HOST_RECORDIO_WRITER_H_
#define DIFACTO_HOST_RECORDIO_WRITER_H_
#include <cstdint>
#include <cstring>
#include <string>
#include "dmlc/logging.h"

namespace difacto {

class RecordIOWriter {
 public:
  static const uint32_t kMagic = 0xced7230a;
  /*! \brief the bytes WriteRecord puts into the file for this payload, appended to *out */
  static void Append(const char* payload, size_t len, std::string* out) {
    CHECK_LT(len, static_cast<size_t>(1) << 29) << "RecordIO only accepts records of less than 2^29 bytes";
    const uint32_t magic = kMagic;
    const size_t lower = (len >> 2U) << 2U;
    size_t dptr = 0;
    auto head = [&](uint32_t cflag, size_t n) {
      const uint32_t lrec = (cflag << 29U) | static_cast<uint32_t>(n);
      out->append(reinterpret_cast<const char*>(&magic), 4);
      out->append(reinterpret_cast<const char*>(&lrec), 4);
    };
    for (size_t i = 0; i < lower; i += 4) {
      uint32_t word;
      memcpy(&word, payload + i, 4);
      if (word != magic) continue;
      head(dptr == 0 ? 1U : 2U, i - dptr);
      out->append(payload + dptr, i - dptr);
      dptr = i + 4;
    }
    head(dptr != 0 ? 3U : 0U, len - dptr);
    out->append(payload + dptr, len - dptr);
    out->append((4 - ((len - dptr) & 3U)) & 3U, '\0');
  }
};

}  // namespace difacto
#endif  // DIFACTO_HOST_RECORDIO_WRITER_H_
