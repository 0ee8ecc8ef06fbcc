// scripted_law_host.cpp -- a scripted opponent's law through the host entry
// (include/satrl_ppo.h: satrl_scripted_act_host) driven from plain C++: the
// arithmetic against a restatement here, both clamp sides, a NaN feature and
// the refusals, on exactly sized heap buffers.  No GPU and no Python in the
// process; `make -C ppo-rl-satellite_amd/csrc asan-host` builds it together
// with csrc/satenv_cpu.cpp under -fsanitize=address,undefined and runs it.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "satrl_ppo.h"

#define REQUIRE(cond)                                                           \
  do {                                                                          \
    if (!(cond)) {                                                              \
      std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond);    \
      return 1;                                                                 \
    }                                                                           \
  } while (0)

// the rule of satrl_ppo.h, written out again (volatile: each product and each
// sum is rounded to f64 on its own whatever this file is compiled with)
static float restated(const satrl_scripted_law& law, const float* s, int d) {
  volatile double acc = law.b[d];
  for (int j = 0; j < 18; ++j) {
    volatile double p = law.G[d][j] * (double)s[j];
    acc = acc + p;
  }
  const double m = law.max_action, a = acc;
  return (float)(a < -m ? -m : (a > m ? m : a));
}

int main() {
  const int64_t n = 37;
  satrl_scripted_law law;
  std::memset(&law, 0, sizeof(law));
  unsigned x = 12345u;
  auto uni = [&]() { x = x * 1664525u + 1013904223u; return (double)(x >> 8) / 16777216.0 - 0.5; };
  for (int d = 0; d < 3; ++d) {
    for (int j = 0; j < 18; ++j) law.G[d][j] = uni() * 1e-3;
    law.b[d] = uni();
  }
  law.G[1][7] = 0.0;                       // (IEEE: 0 * NaN is NaN, a zero weight does not mask a NaN feature)
  law.max_action = 1.6;
  std::vector<float> obs((size_t)n * 18), act((size_t)n * 3, -7.0f);
  for (size_t k = 0; k < obs.size(); ++k) obs[k] = (float)(uni() * (k % 18 < 3 ? 2e3 : 20.0));
  for (int j = 0; j < 18; ++j) obs[1 * 18 + j] = 1e7f;        // rows that saturate either side
  for (int j = 0; j < 18; ++j) obs[2 * 18 + j] = -1e7f;
  obs[3 * 18 + 7] = NAN;
  REQUIRE(satrl_scripted_act_host(n, obs.data(), &law, act.data()) == 0);
  int sat = 0;
  for (int64_t i = 0; i < n; ++i)
    for (int d = 0; d < 3; ++d) {
      const float want = restated(law, &obs[(size_t)i * 18], d), got = act[(size_t)i * 3 + d];
      REQUIRE(std::memcmp(&want, &got, sizeof(float)) == 0 || (std::isnan(want) && std::isnan(got)));
      sat += std::fabs(got) == 1.6f;
    }
  REQUIRE(sat >= 6);
  REQUIRE(std::isnan(act[3 * 3 + 0]) && std::isnan(act[3 * 3 + 1]) && std::isnan(act[3 * 3 + 2]));
  for (int d = 0; d < 3; ++d) REQUIRE(!std::isnan(act[4 * 3 + d]));          // ... and stays in its row

  // a zero law commands nothing
  std::memset(&law, 0, sizeof(law));
  law.max_action = 1.6;
  obs[3 * 18 + 7] = 1.0f;
  REQUIRE(satrl_scripted_act_host(n, obs.data(), &law, act.data()) == 0);
  for (float a : act) REQUIRE(a == 0.0f);

  // refusals
  REQUIRE(satrl_scripted_act_host(0, obs.data(), &law, act.data()) == -1);
  REQUIRE(satrl_scripted_act_host(-1, obs.data(), &law, act.data()) == -1);
  REQUIRE(satrl_scripted_act_host(n, nullptr, &law, act.data()) == -1);
  REQUIRE(satrl_scripted_act_host(n, obs.data(), nullptr, act.data()) == -1);
  REQUIRE(satrl_scripted_act_host(n, obs.data(), &law, nullptr) == -1);
  std::puts("scripted_law_host ok");
  return 0;
}
