// philox_core.h -- the Philox4x32-10 block function and the engine's key
// schedule, for both targets: the gfx950 kernels (the sampling kernels through
// philox_device.h, the env kernels' reset draw through satenv_step.h) and the
// host build of the env ABI (satenv_cpu.cpp, g++).  Integer arithmetic only,
// so both targets give the same words; the rounds reproduce the Random123
// known-answer vectors (tests/test_reset_dist_cpu.py).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PHILOX_HD __host__ __device__ __forceinline__
#else
#define PHILOX_HD static inline
#endif

PHILOX_HD void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int rnd = 0; rnd < 10; ++rnd) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    c[0] = n0;
    c[1] = (uint32_t)p1;
    c[2] = n2;
    c[3] = (uint32_t)p0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}

// key of (seed, stream): streams 0 / 1 are the two agents' action noise, 2 the
// env's reset draw
PHILOX_HD void philox_key(uint64_t seed, uint32_t agent, uint32_t& k0, uint32_t& k1) {
  k0 = (uint32_t)seed ^ (agent * 0x85EBCA6Bu);
  k1 = (uint32_t)(seed >> 32) ^ (agent * 0xC2B2AE35u + 0x27D4EB2Fu);
}
