// swt_philox.h -- the one counter-based generator of the library: Philox4x32-10 of Random123.  The masked-LM draws (swt_mlm.hip)
// and the BPE-dropout draws (swt_bpe_encode.hip) are functions of a position and (seed, epoch) through it and of nothing else;
// tests/mlm_cases.py holds the same function in NumPy.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace swt {

struct Philox {
  uint32_t x[4];
};

// Philox4x32-10 of Random123: the counter (c0, c1, c2, c3) under the key (k0, k1)
__host__ __device__ inline Philox philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; r++) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return Philox{{c0, c1, c2, c3}};
}

}  // namespace swt
