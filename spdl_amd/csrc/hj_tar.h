// hj_tar.h -- the member walk over an in-memory tar archive behind
// spdl_hj_tar_index (include/spdl_hipjpeg.h).  Host only: no HIP include, so
// tests/native/tar_sweep.cpp runs it alone under sanitizers.
#pragma once

#include <cstddef>
#include <cstdint>

namespace hj {

// The parameters of spdl_hj_tar_index, already checked against null.
void tar_index(const uint8_t* data, size_t size, size_t start, int32_t max_entries,
               int64_t* offsets, int64_t* sizes, int64_t* name_offs, char* names, size_t names_cap,
               int32_t* n_out, size_t* next_pos);

}  // namespace hj
