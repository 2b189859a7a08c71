// acc_cells.h -- what the accumulator kernels (acc.hip, moments.hip) read per row: the FILTER bit and the argument cell, widened to the state's class.
#pragma once
#include "int128.h"

namespace dfgpu {

constexpr uint32_t GID_NONE = 0xFFFFFFFFu;

__device__ inline bool filter_pass(const uint64_t* fbits, const uint64_t* fvalid, int64_t i) {
  return fbits == nullptr || (bit_get(fbits, i) && valid_at(fvalid, i));
}
__device__ inline i128 acc_cell_int(const ColView& c, int64_t r) {
  switch (c.type) {
    case DFGPU_INT8: return ((const int8_t*)c.values)[r]; case DFGPU_INT16: return ((const int16_t*)c.values)[r];
    case DFGPU_INT32: case DFGPU_DATE32: return ((const int32_t*)c.values)[r]; case DFGPU_INT64: return ((const int64_t*)c.values)[r];
    case DFGPU_UINT8: return ((const uint8_t*)c.values)[r]; case DFGPU_UINT16: return ((const uint16_t*)c.values)[r];
    case DFGPU_UINT32: return ((const uint32_t*)c.values)[r]; case DFGPU_UINT64: return (i128)((const uint64_t*)c.values)[r];
    case DFGPU_DECIMAL128: return load_i128(c.values, r);
    default: return 0;
  }
}
__device__ inline double acc_cell_f64(const ColView& c, int64_t r) { return c.type == DFGPU_FLOAT32 ? (double)((const float*)c.values)[r] : ((const double*)c.values)[r]; }

}  // namespace dfgpu
