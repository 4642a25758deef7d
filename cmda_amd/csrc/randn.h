// randn.h -- the counter-based normal generator shared by isr_augment.hip (fields 0..2: the ISR noise) and cow_mask.hip (field 3).
#pragma once
#include "common.h"

namespace {

// Philox4x32-10 (Salmon et al., SC'11): key = the 64-bit seed, counter = (pixel / 4, sample, offset low word, 4 * offset high + field).
// Box-Muller on the four words gives the normals of pixels 4q .. 4q+3.  Contraction is off so that every kernel that inlines this
// function computes the same bits.
static __device__ __forceinline__ void randn4(unsigned long long seed, long long offset, int b, int field, unsigned q, float (&n)[4]) {
#pragma clang fp contract(off)
  unsigned c0 = q, c1 = (unsigned)b, c2 = (unsigned)offset, c3 = ((unsigned)((unsigned long long)offset >> 32) << 2) | (unsigned)field;
  unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
    c0 = n0, c1 = n1, c2 = n2, c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  const float s24 = 5.9604644775390625e-8f;   // 2^-24: u in (0, 1), never 0
  const float u0 = ((float)(c0 >> 8) + 0.5f) * s24, u1 = ((float)(c1 >> 8) + 0.5f) * s24;
  const float u2 = ((float)(c2 >> 8) + 0.5f) * s24, u3 = ((float)(c3 >> 8) + 0.5f) * s24;
  const float r0 = sqrtf(-2.f * logf(u0)), r1 = sqrtf(-2.f * logf(u2));
  const float a0 = 6.283185307179586f * u1, a1 = 6.283185307179586f * u3;
  n[0] = r0 * cosf(a0);
  n[1] = r0 * sinf(a0);
  n[2] = r1 * cosf(a1);
  n[3] = r1 * sinf(a1);
}

}  // namespace
