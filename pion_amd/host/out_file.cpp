// out_file.cpp -- see out_file.h
#include "out_file.h"

#include <fcntl.h>
#include <unistd.h>

#include <cerrno>
#include <cstdio>
#include <cstring>

#include "../../include/pion_gpu.h"

namespace pion_host {

std::string fmt_d(double x)
{
  char b[64];
  snprintf(b, sizeof b, "%.17g", x);
  return b;
}

PartFile::PartFile(const char *who, const char *path, std::string &err)
    : who_(who), path_(path), tmp_(path_ + ".part"), err_(err), fd_(open(tmp_.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644))
{
  if (fd_ < 0) err_ = who_ + ": cannot create " + tmp_ + ": " + strerror(errno);
}

PartFile::~PartFile()
{
  if (fd_ < 0) return;
  close(fd_);
  unlink(tmp_.c_str());
}

int PartFile::resize(long total) { return (ftruncate(fd_, (off_t)total) != 0) ? PION_GPU_EINVAL : 0; }

int PartFile::write(const void *p, size_t n, long off)
{
  const char *c = (const char *)p;
  while (n > 0) {
    const ssize_t w = pwrite(fd_, c, n, (off_t)off);
    if (w < 0 && errno == EINTR) continue;
    if (w <= 0) return PION_GPU_EINVAL;
    c += w, off += w, n -= (size_t)w;
  }
  return 0;
}

int PartFile::commit(int rc)
{
  if (rc && err_.empty()) err_ = who_ + ": writing " + tmp_ + " failed: " + strerror(errno);
  close(fd_);
  fd_ = -1;
  if (!rc && rename(tmp_.c_str(), path_.c_str()) != 0) {
    err_ = who_ + ": cannot rename to " + path_ + ": " + strerror(errno);
    rc = PION_GPU_EINVAL;
  }
  if (rc) unlink(tmp_.c_str());
  return rc;
}

}  // namespace pion_host
