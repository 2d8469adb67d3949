// hj_probe.h -- the host header probe (replaces nvjpegGetImageInfo): the SOF
// fields and the scan structure, read from the markers alone.  Host only, no
// HIP runtime: tests/native/header_sweep.cpp links it as it is.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/spdl_hipjpeg.h"

namespace hj {

// Components of the first scan (SOS Ns) after `pos`; 255 when no SOS header
// follows (the device parse then reports the file).
int first_scan_components(const uint8_t* d, size_t size, size_t pos);

// The frame as its last SOF before the first SOS states it (the device parser
// and the oracle keep the last one too), the frame's colour model
// (frame_color: the APP14 Adobe flag seen before that SOF, the component ids)
// and whether the multi-scan path decodes the file.
int probe(const uint8_t* d, size_t size, spdl_hj_image_info* info);

// The EXIF orientation of a file, 1..8 (spdl_hj_get_orientation's rules):
// tag 0x0112 of IFD0 of the first Exif APP1 ahead of the first SOS; 1 for
// whatever is absent, malformed or out of range.  It never fails and reads
// nothing outside [d, d + size).
int exif_orientation(const uint8_t* d, size_t size);

// EXIF orientation 1..8 -> orientation code 0..7 (spdl_hj_orient_code); -1 else.
int orient_code(int exif);

}  // namespace hj
