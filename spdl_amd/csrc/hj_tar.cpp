// hj_tar.cpp -- tar (ustar / GNU 'L' long names / pax 'x' path).
// Same member walk as the reference's InMemoryTarParserImpl::parse_next
// (src/spdl/io/lib/archive/tar_iterator.cpp:125-195): a header that fails the
// magic/checksum test is skipped 512 bytes at a time; an empty name ends the
// archive; 'L' and 'x' records name the next regular file; other types are
// skipped with their payload; a member running past the buffer ends the walk.
#include "hj_tar.h"

#include <cstring>
#include <string>

namespace hj {
namespace {

uint64_t tar_octal(const uint8_t* s, size_t n) {
  uint64_t r = 0;
  for (size_t i = 0; i < n && s[i] != 0 && s[i] != ' '; i++)
    if (s[i] >= '0' && s[i] <= '7') r = r * 8 + (s[i] - '0');
  return r;
}

bool tar_header_ok(const uint8_t* h) {
  if (memcmp(h + 257, "ustar", 5) != 0) return false;
  uint32_t sum = 0;
  for (int i = 0; i < 512; i++) sum += (i >= 148 && i < 156) ? (uint32_t)' ' : h[i];
  return tar_octal(h + 148, 8) == sum;
}

std::string tar_pax_path(const uint8_t* d, size_t n) {
  // records "<len> key=value\n"
  size_t pos = 0;
  while (pos < n) {
    const void* sp = memchr(d + pos, ' ', n - pos);
    if (!sp) break;
    const size_t rs = (size_t)(static_cast<const uint8_t*>(sp) - d) + 1;
    if (rs + 5 <= n && memcmp(d + rs, "path=", 5) == 0) {
      const void* nl = memchr(d + rs + 5, '\n', n - rs - 5);
      if (nl) return std::string((const char*)d + rs + 5,
                                 (size_t)(static_cast<const uint8_t*>(nl) - (d + rs + 5)));
    }
    const void* nl = memchr(d + pos, '\n', n - pos);
    if (!nl) break;
    pos = (size_t)(static_cast<const uint8_t*>(nl) - d) + 1;
  }
  return std::string();
}

}  // namespace

void tar_index(const uint8_t* data, size_t size, size_t start, int32_t max_entries,
               int64_t* offsets, int64_t* sizes, int64_t* name_offs, char* names, size_t names_cap,
               int32_t* n_out, size_t* next_pos) {
  size_t pos = start, used = 0;
  int32_t n = 0;
  std::string pending;
  bool at_end = false;
  while (n < max_entries) {
    const size_t entry_pos = pos;  // resume point if this entry does not fit
    std::string path;
    bool found = false;
    pending.clear();
    while (pos + 512 <= size) {
      const uint8_t* h = data + pos;
      if (!tar_header_ok(h)) {
        pos += 512;
        continue;
      }
      std::string fp;
      if (h[0]) {
        if (h[345]) {
          fp.assign((const char*)h + 345, strnlen((const char*)h + 345, 155));
          if (fp.back() != '/') fp += '/';
        }
        fp.append((const char*)h, strnlen((const char*)h, 100));
      }
      if (fp.empty() && pending.empty()) {
        at_end = true;
        break;
      }
      const uint64_t fsz = tar_octal(h + 124, 12);
      const uint64_t padded = (fsz + 511) & ~511ull;
      const char type = (char)h[156];
      if (type == 'L' || type == 'x') {
        pos += 512;
        if (pos + fsz > size) {
          at_end = true;
          break;
        }
        if (type == 'L') {
          pending.assign((const char*)data + pos, (size_t)fsz);
          if (!pending.empty() && pending.back() == '\0') pending.pop_back();
        } else {
          pending = tar_pax_path(data + pos, (size_t)fsz);
        }
        pos += padded;
        continue;
      }
      if (type == '0' || type == '\0') {
        pos += 512;
        if (!pending.empty()) fp = pending;
        if (pos + fsz > size) {
          at_end = true;
          break;
        }
        path = fp;
        offsets[n] = (int64_t)pos;
        sizes[n] = (int64_t)fsz;
        pos += padded;
        found = true;
        break;
      }
      pending.clear();
      pos += 512 + padded;
    }
    if (!found) {
      if (!at_end) pos = size;
      break;
    }
    if (names && name_offs) {
      if (used + path.size() + 1 > names_cap) {
        pos = entry_pos;  // retry this entry with a fresh names buffer
        break;
      }
      memcpy(names + used, path.c_str(), path.size() + 1);
      name_offs[n] = (int64_t)used;
      used += path.size() + 1;
    }
    n++;
  }
  *n_out = n;
  *next_pos = at_end ? size : pos;
}

}  // namespace hj
