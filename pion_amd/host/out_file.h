// out_file.h -- the file mechanics of every writer of the C++ host loop (write_snapshot, write_fits, write_projection,
// write_columns), stated once.  A file is written under "<path>.part" and renamed when it is whole: one that replaces
// an older one -- a checkpoint -- is whole or absent, and a failure leaves nothing behind.
#ifndef PION_OUT_FILE_H
#define PION_OUT_FILE_H

#include <cstddef>
#include <string>

namespace pion_host {

// a double as every header spells it: %.17g, read back bit for bit
std::string fmt_d(double x);

class PartFile {
 public:
  // opens "<path>.part"; `who` starts every text, e.g. "write_fits".  On failure !ok(), and err holds
  // "<who>: cannot create <tmp>: <strerror>"
  PartFile(const char *who, const char *path, std::string &err);
  // closes, and removes the ".part" file of an object that was not committed
  ~PartFile();
  PartFile(const PartFile &) = delete;
  bool ok() const { return fd_ >= 0; }
  // the file at its final length: what no write covers reads as zero bytes
  int resize(long total);
  // all n bytes at offset off.  0 or PION_GPU_EINVAL, as resize; neither sets a text (commit does)
  int write(const void *p, size_t n, long off);
  // The end of a writer, with the rc of everything it did since the file was opened.  rc != 0: the file is removed, and
  // where no text is set yet -- a backend's failure sets its own -- err becomes "<who>: writing <tmp> failed:
  // <strerror>".  rc == 0: renamed to <path>, or "<who>: cannot rename to <path>: <strerror>" and PION_GPU_EINVAL.
  // Returns the writer's rc
  int commit(int rc);

 private:
  const std::string who_, path_, tmp_;
  std::string &err_;
  int fd_;
};

}  // namespace pion_host
#endif
