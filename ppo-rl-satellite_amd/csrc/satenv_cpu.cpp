// satenv_cpu.cpp -- host build of the environment ABI (include/satenv_cpu.h).
//
// The env step of the gfx950 kernels, compiled by g++ for host cores: the
// same satenv_device.h / satenv_step.h source, one loop iteration per env
// where the kernel has one lane per env, OpenMP over envs.  Same state
// layout as a device handle (f64 planes [16][N], i32 planes [4][N]), so the
// get/set_state planes are interchangeable between the two builds; the
// reset distribution and the per-env episode index likewise (satenv.h).
//
// Reference (qiaobeibei/PPO-RL-Satellite): environment.py:26-255 (ctor,
// reset, step Flag 0/1), CPPO_main.py:119-153 (the loop step_autoreset
// stands for), satellite_function.py:18-99,161-255,317-373,462-565 (the
// danger-zone count with fsolve's MINPACK hybrd).
#include <omp.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "satenv_cpu.h"
#include "satenv_device.h"
#include "satenv_step.h"
#include "satrl_error.h"       // satrl_scripted_act_host's refusals (the satrl_* slot)
#include "scripted_device.h"   // satrl_scripted_act_host (include/satrl_ppo.h)

using namespace satenv;

namespace {

thread_local std::string g_last_error;

int fail(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}

}  // namespace

struct satenv_cpu_env {
  int64_t n = 0;
  int threads = 1;
  satenv_params prm{};
  std::vector<double> f64;
  std::vector<int32_t> i32;
  int32_t err = 0;
  ResetDist rd{};                   // the reset distribution as the step reads it
  satenv_reset_dist dist{};         // ... and as satenv_cpu_set_reset_dist was given it
  ActNoise an{};                    // the actuation noise as the step reads it
  satenv_act_noise noise{};         // ... and as satenv_cpu_set_act_noise was given it
  ObsNoise on{};                    // the observation noise as the step and the reset read it
  satenv_obs_noise obsn{};          // ... and as satenv_cpu_set_obs_noise was given it
};

namespace {

// step_lane for env i; st (may be null) = the four per-env stat planes [4][n]
void step_env(satenv_cpu_env* h, const StepIO& io, int64_t i, bool autoreset, double* st) {
  StepStats s;
  const int rc = step_lane<true, true, true, true>(h->prm, h->n, h->f64.data(), h->i32.data(), io, i, autoreset, s);
  if (rc) {
#pragma omp critical(satenv_cpu_err)
    if (h->err == 0) h->err = rc;
  }
  if (st) {
    const int64_t n = h->n;
    st[i] = s.fin;
    st[n + i] = s.fin_ret;
    st[2 * n + i] = s.rew;
    st[3 * n + i] = s.cap;
  }
}

}  // namespace

extern "C" {

const char* satenv_cpu_last_error(void) { return g_last_error.c_str(); }

int satenv_cpu_create(satenv_cpu_env** out, int64_t num_envs, const satenv_params* p, int device) {
  if (!out || !p || num_envs <= 0 || device < 0) return fail(SATENV_ERR_ARG, "satenv_cpu_create: bad arguments");
  if (!params_ok(*p)) return fail(SATENV_ERR_ARG, "satenv_cpu_create: propagator must be 0/1/2, rk4_substeps >= 1");
  satenv_cpu_env* h = new satenv_cpu_env();
  h->n = num_envs;
  h->threads = device > 0 ? device : omp_get_max_threads();
  h->prm = *p;
  h->f64.assign((size_t)kF64Planes * num_envs, 0.0);
  h->i32.assign((size_t)kI32Planes * num_envs, 0);
  satenv_cpu_default_reset_dist(&h->dist);
  reset_dist_pack(h->dist, h->rd);
  satenv_cpu_default_obs_noise(&h->obsn);
  obs_noise_pack(h->obsn, h->on);
  for (int64_t i = 0; i < num_envs; ++i) init_env(h->prm, num_envs, h->f64.data(), h->i32.data(), i);
  *out = h;
  return SATENV_OK;
}

int satenv_cpu_destroy(satenv_cpu_env* h) {
  delete h;
  return SATENV_OK;
}

int satenv_cpu_num_envs(const satenv_cpu_env* h, int64_t* n) {
  if (!h || !n) return fail(SATENV_ERR_ARG, "satenv_cpu_num_envs: null");
  *n = h->n;
  return SATENV_OK;
}

int satenv_cpu_set_params(satenv_cpu_env* h, const satenv_params* p) {
  if (!h || !p) return fail(SATENV_ERR_ARG, "satenv_cpu_set_params: null");
  if (!params_ok(*p)) return fail(SATENV_ERR_ARG, "satenv_cpu_set_params: propagator must be 0/1/2, rk4_substeps >= 1");
  const int32_t flag = h->prm.flag;
  h->prm = *p;
  h->prm.flag = flag;
  return SATENV_OK;
}

int satenv_cpu_reset(satenv_cpu_env* h, int32_t flag, const uint8_t* env_mask, float* obs_out, double* obs64_out,
                     void* /*stream*/) {
  if (!h) return fail(SATENV_ERR_ARG, "satenv_cpu_reset: null handle");
  if (flag < 0 || flag > 2) return fail(SATENV_ERR_ARG, "satenv_cpu_reset: Flag must be 0, 1 or 2");
  h->prm.flag = flag;
#pragma omp parallel for num_threads(h->threads) schedule(static)
  for (int64_t i = 0; i < h->n; ++i)
    reset_env<true>(h->prm, &h->rd, h->n, h->f64.data(), h->i32.data(), flag, env_mask, obs_out, obs64_out, i,
                    &h->on);
  return SATENV_OK;
}

int satenv_cpu_step(satenv_cpu_env* h, const float* pa, const float* ea, const int32_t* episode_count,
                    float* obs_out, double* obs64_out, double* reward_out, uint8_t* done_out, void* /*stream*/) {
  if (!h || !pa || !ea) return fail(SATENV_ERR_ARG, "satenv_cpu_step: null argument");
  const StepIO io{pa, ea, episode_count, obs_out, obs64_out, reward_out, nullptr, done_out, nullptr, nullptr, &h->rd,
                  &h->an, &h->on};
#pragma omp parallel for num_threads(h->threads) schedule(dynamic, 64)
  for (int64_t i = 0; i < h->n; ++i) step_env(h, io, i, false, nullptr);
  return SATENV_OK;
}

int satenv_cpu_step_autoreset(satenv_cpu_env* h, const float* pa, const float* ea, float* obs_out,
                              float* reward_out, uint8_t* done_out, double* stats_out, void* /*stream*/) {
  if (!h || !pa || !ea) return fail(SATENV_ERR_ARG, "satenv_cpu_step_autoreset: null argument");
  const StepIO io{pa, ea, nullptr, obs_out, nullptr, nullptr, reward_out, done_out, nullptr, nullptr, &h->rd,
                  &h->an, &h->on};
  const int64_t n = h->n;
  std::vector<double> st;
  if (stats_out) st.assign((size_t)4 * n, 0.0);
  double* s = stats_out ? st.data() : nullptr;
#pragma omp parallel for num_threads(h->threads) schedule(dynamic, 64)
  for (int64_t i = 0; i < n; ++i) step_env(h, io, i, true, s);
  if (stats_out) {            // the kernel's per-wave sums, here in env order (deterministic)
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < 4; ++k)
      for (int64_t i = 0; i < n; ++i) acc[k] += s[k * n + i];
    for (int k = 0; k < 4; ++k)
      if (k == 2 || acc[k] != 0.0) stats_out[k] += acc[k];
  }
  return SATENV_OK;
}

int satenv_cpu_get_state(const satenv_cpu_env* h, double* f64_planes, int32_t* i32_planes, void* /*stream*/) {
  if (!h) return fail(SATENV_ERR_ARG, "satenv_cpu_get_state: null handle");
  if (f64_planes) std::memcpy(f64_planes, h->f64.data(), sizeof(double) * SATENV_F64_PLANES * h->n);
  if (i32_planes) std::memcpy(i32_planes, h->i32.data(), sizeof(int32_t) * SATENV_I32_PLANES * h->n);
  return SATENV_OK;
}

int satenv_cpu_set_state(satenv_cpu_env* h, const double* f64_planes, const int32_t* i32_planes, void* /*stream*/) {
  if (!h) return fail(SATENV_ERR_ARG, "satenv_cpu_set_state: null handle");
  if (f64_planes) std::memcpy(h->f64.data(), f64_planes, sizeof(double) * SATENV_F64_PLANES * h->n);
  if (i32_planes) std::memcpy(h->i32.data(), i32_planes, sizeof(int32_t) * SATENV_I32_PLANES * h->n);
  return SATENV_OK;
}

int satenv_cpu_default_reset_dist(satenv_reset_dist* d) {
  if (!d) return fail(SATENV_ERR_ARG, "satenv_cpu_default_reset_dist: null");
  std::memset(d, 0, sizeof(*d));
  double k[12];
  reset_kin(satenv_params{}, k);
  std::memcpy(d->lo, k, sizeof(k));
  std::memcpy(d->hi, k, sizeof(k));
  return SATENV_OK;
}

int satenv_cpu_set_reset_dist(satenv_cpu_env* h, const satenv_reset_dist* d, void* /*stream*/) {
  if (!h || !d) return fail(SATENV_ERR_ARG, "satenv_cpu_set_reset_dist: null argument");
  ResetDist rd;
  if (!reset_dist_pack(*d, rd))
    return fail(SATENV_ERR_ARG, "satenv_cpu_set_reset_dist: bounds must be finite, lo <= hi");
  h->rd = rd;
  h->dist = *d;
  h->dist.enabled = d->enabled != 0;
  h->dist.reserved = 0;
  return SATENV_OK;
}

int satenv_cpu_get_reset_dist(const satenv_cpu_env* h, satenv_reset_dist* d) {
  if (!h || !d) return fail(SATENV_ERR_ARG, "satenv_cpu_get_reset_dist: null argument");
  *d = h->dist;
  return SATENV_OK;
}

int satenv_cpu_default_act_noise(satenv_act_noise* d) {
  if (!d) return fail(SATENV_ERR_ARG, "satenv_cpu_default_act_noise: null");
  std::memset(d, 0, sizeof(*d));
  return SATENV_OK;
}

int satenv_cpu_set_act_noise(satenv_cpu_env* h, const satenv_act_noise* d, void* /*stream*/) {
  if (!h || !d) return fail(SATENV_ERR_ARG, "satenv_cpu_set_act_noise: null argument");
  ActNoise an;
  if (const char* bad = act_noise_pack(*d, an))
    return fail(SATENV_ERR_ARG, std::string("satenv_cpu_set_act_noise: ") + bad);
  h->an = an;
  h->noise = *d;
  h->noise.enabled = d->enabled != 0;
  h->noise.reserved = 0;
  return SATENV_OK;
}

int satenv_cpu_get_act_noise(const satenv_cpu_env* h, satenv_act_noise* d) {
  if (!h || !d) return fail(SATENV_ERR_ARG, "satenv_cpu_get_act_noise: null argument");
  *d = h->noise;
  return SATENV_OK;
}

int satenv_cpu_act_noise_host(const satenv_act_noise* d, int64_t gid, int32_t ep, int32_t cnt, int32_t agent,
                              const float a_in[3], float a_out[3]) {
  if (const char* bad = act_noise_host(d, gid, ep, cnt, agent, a_in, a_out))
    return fail(SATENV_ERR_ARG, std::string("satenv_cpu_act_noise_host: ") + bad);
  return SATENV_OK;
}

int satenv_cpu_default_obs_noise(satenv_obs_noise* d) {
  if (!d) return fail(SATENV_ERR_ARG, "satenv_cpu_default_obs_noise: null");
  std::memset(d, 0, sizeof(*d));
  d->hold = 1;
  return SATENV_OK;
}

int satenv_cpu_set_obs_noise(satenv_cpu_env* h, const satenv_obs_noise* d, void* /*stream*/) {
  if (!h || !d) return fail(SATENV_ERR_ARG, "satenv_cpu_set_obs_noise: null argument");
  ObsNoise on;
  if (const char* bad = obs_noise_pack(*d, on))
    return fail(SATENV_ERR_ARG, std::string("satenv_cpu_set_obs_noise: ") + bad);
  h->on = on;
  h->obsn = *d;
  h->obsn.enabled = d->enabled != 0;
  return SATENV_OK;
}

int satenv_cpu_get_obs_noise(const satenv_cpu_env* h, satenv_obs_noise* d) {
  if (!h || !d) return fail(SATENV_ERR_ARG, "satenv_cpu_get_obs_noise: null argument");
  *d = h->obsn;
  return SATENV_OK;
}

int satenv_cpu_obs_noise_host(const satenv_obs_noise* d, int64_t gid, int32_t ep, int32_t cnt,
                              const double k_in[12], double k_out[12], float obs_out[18]) {
  if (const char* bad = obs_noise_host(d, gid, ep, cnt, k_in, k_out, obs_out))
    return fail(SATENV_ERR_ARG, std::string("satenv_cpu_obs_noise_host: ") + bad);
  return SATENV_OK;
}

int satenv_cpu_get_episode_index(const satenv_cpu_env* h, int32_t* out, void* /*stream*/) {
  if (!h || !out) return fail(SATENV_ERR_ARG, "satenv_cpu_get_episode_index: null argument");
  std::memcpy(out, h->i32.data() + (size_t)kPlaneEp * h->n, sizeof(int32_t) * h->n);
  return SATENV_OK;
}

int satenv_cpu_set_episode_index(satenv_cpu_env* h, const int32_t* in, void* /*stream*/) {
  if (!h) return fail(SATENV_ERR_ARG, "satenv_cpu_set_episode_index: null handle");
  int32_t* dst = h->i32.data() + (size_t)kPlaneEp * h->n;
  if (in) std::memcpy(dst, in, sizeof(int32_t) * h->n);
  else std::memset(dst, 0, sizeof(int32_t) * h->n);
  return SATENV_OK;
}

int satenv_cpu_get_episode_return(const satenv_cpu_env* h, double* out, void* /*stream*/) {
  if (!h || !out) return fail(SATENV_ERR_ARG, "satenv_cpu_get_episode_return: null argument");
  std::memcpy(out, h->f64.data() + (size_t)kPlaneRet * h->n, sizeof(double) * h->n);
  return SATENV_OK;
}

int satenv_cpu_set_episode_return(satenv_cpu_env* h, const double* in, void* /*stream*/) {
  if (!h) return fail(SATENV_ERR_ARG, "satenv_cpu_set_episode_return: null handle");
  double* dst = h->f64.data() + (size_t)kPlaneRet * h->n;
  if (in) std::memcpy(dst, in, sizeof(double) * h->n);
  else std::memset(dst, 0, sizeof(double) * h->n);
  return SATENV_OK;
}

int satenv_cpu_danger_zone(int64_t n, const double* states, const double* fuel, const int32_t* fuel_mode,
                           int32_t* count_out, void* /*stream*/) {
  if (n <= 0 || !states || !fuel || !fuel_mode || !count_out)
    return fail(SATENV_ERR_ARG, "satenv_cpu_danger_zone: bad args");
  satenv_params prm;
  std::memset(&prm, 0, sizeof(prm));                      // states are absolute: R_cw = V_cw = 0
#pragma omp parallel for schedule(dynamic, 64)
  for (int64_t i = 0; i < n; ++i) {
    int cnt = 0;
    const int rc = danger_zone(prm, states + i * 12, fuel[i], fuel_mode[i], cnt);
    count_out[i] = rc ? rc : cnt;
  }
  return SATENV_OK;
}

int satenv_cpu_check(satenv_cpu_env* h, int32_t* status) {
  if (!h || !status) return fail(SATENV_ERR_ARG, "satenv_cpu_check: null");
  *status = h->err;
  return SATENV_OK;
}

// A scripted opponent's law on host pointers (include/satrl_ppo.h): the
// kernels' own source, one loop iteration per env row, no device call.
int satrl_scripted_act_host(int64_t N, const float* obs, const satrl_scripted_law* law, float* act) {
  if (N <= 0) return satrl_err::fail(-1, __func__, "N " + std::to_string(N) + " <= 0");
  if (int rc = satrl_err::null_arg(__func__, SATRL_PTRS(obs, law, act))) return rc;
  for (int64_t i = 0; i < N; ++i) satrl_scripted::law_row(law, obs + i * 18, act + i * 3);
  return 0;
}

}  // extern "C"
