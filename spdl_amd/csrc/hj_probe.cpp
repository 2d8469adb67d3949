// hj_probe.cpp -- the host header probe (see hj_probe.h).
#include "hj_probe.h"

#include <string.h>

#include "hj_common.h"

namespace hj {

int first_scan_components(const uint8_t* d, size_t size, size_t pos) {
  for (;;) {
    while (pos < size && d[pos] != 0xFF) pos++;
    while (pos < size && d[pos] == 0xFF) pos++;
    if (pos >= size) return 255;
    const int m = d[pos++];
    if (m == 0x01 || (m >= 0xD0 && m <= 0xD8)) continue;
    if (m == 0xD9 || pos + 3 > size) return 255;
    if (m == 0xDA) return d[pos + 2];
    pos += (size_t)((d[pos] << 8) | d[pos + 1]);
  }
}

// ---- host SOF probe (replaces nvjpegGetImageInfo) --------------------------
// A file may hold several SOF segments ahead of its first scan: the walk goes
// on to the first SOS and the last SOF before it is the frame.  What ends the
// walk after a SOF without a scan header (EOI, a broken segment, the end of
// the file) is left to the device parse, which reports the file.
int probe(const uint8_t* d, size_t size, spdl_hj_image_info* info) {
  memset(info, 0, sizeof(*info));
  if (!d || size < 4 || d[0] != 0xFF || d[1] != 0xD8) return SPDL_HJ_ERR_NOT_JPEG;
  size_t pos = 2, sof_end = 0;
  int adobe = -1, sof = 0;  // sof: the marker of the last SOF (0: none yet)
  for (;;) {
    while (pos < size && d[pos] != 0xFF) pos++;
    while (pos < size && d[pos] == 0xFF) pos++;
    if (pos >= size) break;
    int m = d[pos++];
    if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;
    if (m == 0xD9 || m == 0xDA) break;  // the first scan, or no scan at all
    if (pos + 2 > size) break;
    int len = (d[pos] << 8) | d[pos + 1];
    if (len < 2 || pos + (size_t)len > size) break;
    const uint8_t* s = d + pos + 2;
    pos += (size_t)len;
    if (m == 0xEE) {
      if (len >= 14 && memcmp(s, "Adobe", 5) == 0) adobe = s[11];
      continue;
    }
    if (m == 0xC0 || m == 0xC1 || m == 0xC2) {  // sequential or progressive Huffman
      if (len < 8) return SPDL_HJ_ERR_BAD_HEADER;
      if (s[0] != 8) return SPDL_HJ_ERR_UNSUPPORTED;
      info->height = (s[1] << 8) | s[2];
      info->width = (s[3] << 8) | s[4];
      info->ncomp = s[5];
      if (info->height == 0) return SPDL_HJ_ERR_UNSUPPORTED;
      if (info->width == 0) return SPDL_HJ_ERR_BAD_HEADER;
      if (info->ncomp != 1 && info->ncomp != 3 && info->ncomp != 4) return SPDL_HJ_ERR_UNSUPPORTED;
      if (len < 8 + 3 * info->ncomp) return SPDL_HJ_ERR_BAD_HEADER;
      int ids[kMaxComp] = {};
      for (int c = 0; c < kMaxComp; c++) info->h_samp[c] = info->v_samp[c] = 0;
      for (int c = 0; c < info->ncomp; c++) {
        ids[c] = s[6 + 3 * c];
        info->h_samp[c] = s[7 + 3 * c] >> 4;
        info->v_samp[c] = s[7 + 3 * c] & 15;
        if (info->h_samp[c] < 1 || info->h_samp[c] > 4 || info->v_samp[c] < 1 ||
            info->v_samp[c] > 4)
          return SPDL_HJ_ERR_BAD_HEADER;
      }
      if (!frame_color(info->ncomp, info->h_samp, info->v_samp, ids, adobe, &info->color))
        return SPDL_HJ_ERR_UNSUPPORTED;
      sof = m;
      sof_end = pos;
      continue;
    }
    if (m == 0xC3 || (m >= 0xC5 && m <= 0xC7) || (m >= 0xC9 && m <= 0xCB) ||
        (m >= 0xCD && m <= 0xCF))
      return SPDL_HJ_ERR_UNSUPPORTED;  // lossless, hierarchical, arithmetic
  }
  if (!sof) return SPDL_HJ_ERR_BAD_HEADER;  // no SOF before the scan
  // the scan structure: progressive, or a first scan with fewer components
  // than the frame (the multi-scan path decodes both)
  info->multiscan = sof == 0xC2 || first_scan_components(d, size, sof_end) < info->ncomp;
  return SPDL_HJ_OK;
}

// ---- EXIF orientation (tag 0x0112 of IFD0) ----------------------------------
namespace {

// The TIFF structure of an Exif APP1 payload behind "Exif\0\0": t[0, n).
// Every read is checked against n; whatever does not hold is orientation 1.
int tiff_orientation(const uint8_t* t, size_t n) {
  if (n < 8) return 1;
  bool le;
  if (t[0] == 'I' && t[1] == 'I' && t[2] == 0x2A && t[3] == 0) le = true;
  else if (t[0] == 'M' && t[1] == 'M' && t[2] == 0 && t[3] == 0x2A) le = false;
  else return 1;
  // (callers have checked off + 2, off + 4 <= n)
  auto rd16 = [&](size_t off) -> uint32_t {
    return le ? (uint32_t)t[off] | (uint32_t)t[off + 1] << 8
              : (uint32_t)t[off] << 8 | (uint32_t)t[off + 1];
  };
  auto rd32 = [&](size_t off) -> uint32_t {
    return le ? rd16(off) | rd16(off + 2) << 16 : rd16(off) << 16 | rd16(off + 2);
  };
  const size_t ifd = rd32(4);
  if (ifd > n || n - ifd < 2) return 1;
  const size_t cnt = rd16(ifd);
  for (size_t i = 0; i < cnt; i++) {
    const size_t e = ifd + 2 + 12 * i;
    if (e > n || n - e < 12) return 1;
    if (rd16(e) != 0x0112) continue;
    const uint32_t type = rd16(e + 2), count = rd32(e + 4);
    if (count != 1 || (type != 3 && type != 4)) return 1;
    const uint32_t v = type == 3 ? rd16(e + 8) : rd32(e + 8);
    return v >= 1 && v <= 8 ? (int)v : 1;
  }
  return 1;
}

}  // namespace

int exif_orientation(const uint8_t* d, size_t size) {
  if (!d || size < 4 || d[0] != 0xFF || d[1] != 0xD8) return 1;
  size_t pos = 2;
  for (;;) {  // (the marker walk of probe)
    while (pos < size && d[pos] != 0xFF) pos++;
    while (pos < size && d[pos] == 0xFF) pos++;
    if (pos >= size) break;
    const int m = d[pos++];
    if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;
    if (m == 0xD9 || m == 0xDA) break;
    if (pos + 2 > size) break;
    const int len = (d[pos] << 8) | d[pos + 1];
    if (len < 2 || pos + (size_t)len > size) break;  // (a truncated segment)
    const uint8_t* s = d + pos + 2;
    const size_t n = (size_t)len - 2;
    pos += (size_t)len;
    // the first Exif APP1 decides (XMP lives in APP1 as well: another prefix)
    if (m == 0xE1 && n >= 6 && memcmp(s, "Exif\0\0", 6) == 0) return tiff_orientation(s + 6, n - 6);
  }
  return 1;
}

int orient_code(int exif) {
  static const int8_t kCode[9] = {-1, 0, 1, 3, 2, 4, 5, 7, 6};
  return exif >= 1 && exif <= 8 ? kCode[exif] : -1;
}

}  // namespace hj

extern "C" {

int spdl_hj_get_orientation(const uint8_t* data, size_t size, int32_t* exif) {
  if (!exif) return SPDL_HJ_ERR_INVALID_ARG;
  *exif = 1;
  spdl_hj_image_info info;
  const int rc = hj::probe(data, size, &info);
  if (rc) return rc;
  *exif = hj::exif_orientation(data, size);
  return SPDL_HJ_OK;
}

int spdl_hj_orient_code(int32_t exif) { return hj::orient_code(exif); }

}  // extern "C"
