// Philox4x32-10 (counter-based; Salmon et al. 2011) and the two uniform conversions of the library's random streams: shared by
// sampling.hip (muse_sample_step's draws, muse_dropout's keep masks) and attention.hip (the same keep masks, drawn in the kernel).
#pragma once
#include <stdint.h>

struct u4 { uint32_t x, y, z, w; };
__device__ __forceinline__ u4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return u4{c0, c1, c2, c3};
}
__device__ __forceinline__ float u01_open_low(uint32_t r) { return ((float)(r >> 8) + 1.0f) * (1.0f / 16777216.0f); }   // (0, 1]
__device__ __forceinline__ float u01_open_high(uint32_t r) { return (float)(r >> 8) * (1.0f / 16777216.0f); }            // [0, 1)

#define MUSE_DROPOUT_TAG 0x6D757365u   // counter word 2 of the dropout stream (word 3 is 0)

// muse_dropout's multipliers (keep / (1 - p) = scale, or 0) of the four elements 4 * blk .. 4 * blk + 3 of the stream (seed, offset):
// one Philox block, for the row kernels that apply nn.Dropout to four consecutive, 4-aligned columns of their own result
__device__ __forceinline__ void dropout_mult4(uint64_t seed, uint64_t offset, uint64_t blk, float p, float scale, float (&m)[4]) {
  const uint64_t c = offset + blk;
  const u4 r = philox4x32_10((uint32_t)c, (uint32_t)(c >> 32), MUSE_DROPOUT_TAG, 0u, (uint32_t)seed, (uint32_t)(seed >> 32));
  m[0] = u01_open_high(r.x) >= p ? scale : 0.0f;
  m[1] = u01_open_high(r.y) >= p ? scale : 0.0f;
  m[2] = u01_open_high(r.z) >= p ? scale : 0.0f;
  m[3] = u01_open_high(r.w) >= p ? scale : 0.0f;
}
