// scripted_device.h -- a scripted opponent's linear guidance law, one source
// for the gfx950 kernels (ppo_kernels.hip) and the host build (g++).
//
//   act[d] = (float) clamp(b[d] + sum_j G[d][j] * (double)s[j], +-max_action)
//
// over the 18 RAW observation features s of one env (metres, m/s; the first
// six are the relative position and velocity, satenv_step.h write_obs).  Per
// (row, d) the arithmetic is fixed: every product is rounded to f64, then
// added to the running sum in ascending j, starting from b[d]; contraction is
// switched off here whatever the translation unit's flags say, so the host
// build, the stand-alone kernel and the fused policy kernel give the same
// bits.  A NaN sum fails both comparisons of the clamp and passes through.
//
// The law block is uniform over a launch: on the device it is read through
// the constant address space (scalar loads, as satenv_step.h rd_load reads
// the reset box), one action dimension's 18 weights at a time -- all 57
// doubles at once would not fit the scalar register file.
#ifndef SATRL_SCRIPTED_DEVICE_H
#define SATRL_SCRIPTED_DEVICE_H
#include <stdint.h>

#include "satrl_ppo.h"

#if defined(__HIPCC__)
#define SATRL_SCRIPTED_HD __host__ __device__ inline
#else
#define SATRL_SCRIPTED_HD inline
#endif
// no fused multiply-add in the law, under any -ffp-contract of the caller
#if defined(__clang__)
#define SATRL_SCRIPTED_NO_CONTRACT
#define SATRL_SCRIPTED_NO_CONTRACT_BODY _Pragma("clang fp contract(off)")
#elif defined(__GNUC__)
#define SATRL_SCRIPTED_NO_CONTRACT __attribute__((optimize("fp-contract=off")))
#define SATRL_SCRIPTED_NO_CONTRACT_BODY
#else
#define SATRL_SCRIPTED_NO_CONTRACT
#define SATRL_SCRIPTED_NO_CONTRACT_BODY
#endif

namespace satrl_scripted {

constexpr int kObs = 18, kAct = 3;

template <class T>
SATRL_SCRIPTED_HD T law_load(const T* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  return *(const __attribute__((address_space(4))) T*)p;
#else
  return *p;
#endif
}

// one env: s = its 18 raw features, act = its 3 actions
SATRL_SCRIPTED_NO_CONTRACT SATRL_SCRIPTED_HD void law_row(const satrl_scripted_law* law, const float* s, float* act) {
  SATRL_SCRIPTED_NO_CONTRACT_BODY
  float x[kObs];                                  // (converted where used: 18 registers, not 36)
#pragma unroll
  for (int j = 0; j < kObs; ++j) x[j] = s[j];
  const double m = law_load(&law->max_action);
#pragma nounroll
  for (int d = 0; d < kAct; ++d) {                // (not unrolled: 18 weights in scalar registers at a time)
    double acc = law_load(&law->b[d]);
#pragma unroll
    for (int j = 0; j < kObs; ++j) {
      const double p = law_load(&law->G[d][j]) * (double)x[j];
      acc = acc + p;
    }
    const double c = acc < -m ? -m : (acc > m ? m : acc);
    act[d] = (float)c;
  }
}

}  // namespace satrl_scripted
#endif
