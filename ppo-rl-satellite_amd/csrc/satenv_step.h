// satenv_step.h -- one environment's init, reset and step (environment.py:
// 26-255) per lane, for both targets: the gfx950 kernels (satenv_kernels.hip)
// and the host build of the same ABI (satenv_cpu.cpp, OpenMP over envs).
// step_lane is the whole step; the multi-wave kernels compose its pieces.
//
// Per-handle state layout (num_envs = N):
//   f64 planes [16][N]  Pp0..2 Pv0..2 Ep0..2 Ev0..2 fuel_c fuel_t dis ep_return
//   i32 planes [4][N]   dangerous_zone, episode_count, bits, episode index
// (the last f64 and the last i32 plane are internal: get/set_state copy the
// public SATENV_F64_PLANES / SATENV_I32_PLANES)
#pragma once
#include <cmath>

#include "philox_core.h"
#include "satenv_device.h"

namespace satenv {

constexpr int kF64Planes = 16;   // 15 public + per-env episode return
constexpr int kI32Planes = 4;   // 3 public + per-env episode index
constexpr int kPlaneRet = 15;
constexpr int kPlaneDz = 0, kPlaneCount = 1, kPlaneBits = 2, kPlaneEp = 3;
constexpr uint32_t kResetStream = 2;   // philox_key stream of the reset draw (0 / 1: the agents' action noise)
constexpr uint32_t kActNoiseStream = 3;   // ... and of agent g's actuation noise: 3 + g
constexpr uint32_t kObsBiasStream = 5;    // ... of the tracking errors' episode bias
constexpr uint32_t kObsNoiseStream = 6;   // ... and of block j of their refreshed part: 6 + j, j = 0, 1, 2

struct alignas(8) F32x2 { float x, y; };

inline bool params_ok(const Params& p) { return p.propagator >= 0 && p.propagator <= 2 && p.rk4_substeps >= 1; }

// The handle's reset distribution as the kernels read it (satenv_reset_dist,
// include/satenv.h): a uniform box over the 12 kinematic scalars, span = hi -
// lo rounded once on the host.  It lives in a small block owned by the handle
// and is read only where an env resets.
struct ResetDist {
  double lo[12], span[12];
  uint32_t k0, k1;        // philox_key(seed, kResetStream)
  int64_t env_offset;     // global env id of env 0
  int32_t enabled;
  int32_t reserved;
};

// satenv_reset_dist -> ResetDist; false where a bound is not finite, lo > hi or hi - lo overflows
inline bool reset_dist_pack(const satenv_reset_dist& in, ResetDist& out) {
  for (int c = 0; c < 12; ++c) {
    const double span = in.hi[c] - in.lo[c];
    if (!std::isfinite(in.lo[c]) || !std::isfinite(in.hi[c]) || !(in.lo[c] <= in.hi[c]) || !std::isfinite(span))
      return false;
    out.lo[c] = in.lo[c];
    out.span[c] = span;
  }
  philox_key(in.seed, kResetStream, out.k0, out.k1);
  out.env_offset = in.env_offset;
  out.enabled = in.enabled != 0;
  out.reserved = 0;
  return true;
}

// The handle's actuation noise as the kernels read it (satenv_act_noise,
// include/satenv.h): per agent g (0 pursuer, 1 evader) the
// half-widths of the thrust magnitude and pointing errors and the key of its
// stream.  A block of its own beside the ResetDist, written by its own setter
// launch and read where step_begin clips the actions.
struct ActNoise {
  double mag[2], dir[2];
  uint32_t k0[2], k1[2];  // philox_key(seed, kActNoiseStream + g)
  int64_t env_offset;     // global env id of env 0
  int32_t enabled;
  int32_t reserved;
};

// satenv_act_noise -> ActNoise; nullptr, or what is wrong with which field
inline const char* act_noise_pack(const satenv_act_noise& in, ActNoise& out) {
  static const char* const kBad[2][3] = {
      {"mag[0] must be finite and >= 0", "dir[0] must be finite and >= 0",
       "mag[0] must not exceed 1 (the thrust direction must not flip)"},
      {"mag[1] must be finite and >= 0", "dir[1] must be finite and >= 0",
       "mag[1] must not exceed 1 (the thrust direction must not flip)"}};
  for (int g = 0; g < 2; ++g) {
    if (!std::isfinite(in.mag[g]) || !(in.mag[g] >= 0.0)) return kBad[g][0];
    if (!std::isfinite(in.dir[g]) || !(in.dir[g] >= 0.0)) return kBad[g][1];
    if (in.mag[g] > 1.0) return kBad[g][2];
    out.mag[g] = in.mag[g];
    out.dir[g] = in.dir[g];
    philox_key(in.seed, kActNoiseStream + (uint32_t)g, out.k0[g], out.k1[g]);
  }
  out.env_offset = in.env_offset;
  out.enabled = in.enabled != 0;
  out.reserved = 0;
  return nullptr;
}

// The handle's observation noise as the kernels read it (satenv_obs_noise,
// include/satenv.h): per tracked craft g the half-widths of
// the episode bias and of the refreshed error on its position and velocity
// scalars, and the keys of the four streams.  A block of its own beside the
// ActNoise, written by its own setter launch and read where a kernel writes
// the f32 observation row.
struct ObsNoise {
  double bias_pos[2], bias_vel[2], pos[2], vel[2];
  uint32_t kb0, kb1;        // philox_key(seed, kObsBiasStream)
  uint32_t kw0[3], kw1[3];  // philox_key(seed, kObsNoiseStream + j)
  int64_t env_offset;       // global env id of env 0
  int32_t hold;             // >= 1
  int32_t enabled;
};

// satenv_obs_noise -> ObsNoise; nullptr, or what is wrong with which field
inline const char* obs_noise_pack(const satenv_obs_noise& in, ObsNoise& out) {
  static const char* const kBad[2][4] = {
      {"bias_pos[0] must be finite and >= 0", "bias_vel[0] must be finite and >= 0",
       "pos[0] must be finite and >= 0", "vel[0] must be finite and >= 0"},
      {"bias_pos[1] must be finite and >= 0", "bias_vel[1] must be finite and >= 0",
       "pos[1] must be finite and >= 0", "vel[1] must be finite and >= 0"}};
  for (int g = 0; g < 2; ++g) {
    const double v[4] = {in.bias_pos[g], in.bias_vel[g], in.pos[g], in.vel[g]};
    for (int f = 0; f < 4; ++f)
      if (!std::isfinite(v[f]) || !(v[f] >= 0.0)) return kBad[g][f];
    out.bias_pos[g] = in.bias_pos[g];
    out.bias_vel[g] = in.bias_vel[g];
    out.pos[g] = in.pos[g];
    out.vel[g] = in.vel[g];
  }
  if (in.hold < 1) return "hold must be >= 1";
  philox_key(in.seed, kObsBiasStream, out.kb0, out.kb1);
  for (int j = 0; j < 3; ++j) philox_key(in.seed, kObsNoiseStream + (uint32_t)j, out.kw0[j], out.kw1[j]);
  out.env_offset = in.env_offset;
  out.hold = in.hold;
  out.enabled = in.enabled != 0;
  return nullptr;
}

struct StepIO {
  const float* pa;
  const float* ea;
  const int32_t* ext_count;   // nullptr -> device counters
  float* obs;
  double* obs64;
  double* rew64;
  float* rew32;
  uint8_t* done;
  double* stats;
  int32_t* err;
  const ResetDist* rd;        // the handle's reset distribution (never null)
  const ActNoise* an;         // the handle's actuation noise (never null)
  const ObsNoise* on;         // the handle's observation noise (never null)
};

// one env's share of a step's statistics (step_autoreset's stats_out): episode
// finished, its return, the step's reward, capture
struct StepStats { double fin = 0.0, fin_ret = 0.0, rew = 0.0, cap = 0.0; };

SATENV_HD void write_obs(float* obs, double* obs64, int64_t i, const double (&k)[12]) {
  // [Pp-Ep, Pv-Ev, Pp, Pv, Ep, Ev]  environment.py:76-77,177-178
  double o[18];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    o[c] = k[c] - k[6 + c];
    o[3 + c] = k[3 + c] - k[9 + c];
    o[6 + c] = k[c];
    o[9 + c] = k[3 + c];
    o[12 + c] = k[6 + c];
    o[15 + c] = k[9 + c];
  }
  if (obs) {
    F32x2* dst = reinterpret_cast<F32x2*>(obs + i * 18);     // 8-B aligned rows
#pragma unroll
    for (int c = 0; c < 9; ++c) dst[c] = F32x2{(float)o[2 * c], (float)o[2 * c + 1]};
  }
  if (obs64) {
#pragma unroll
    for (int c = 0; c < 18; ++c) obs64[i * 18 + c] = o[c];
  }
}

SATENV_HD void reset_kin(const Params& /*p*/, double (&k)[12]) {
  // environment.py:67-71 reset positions/velocities (int64 arrays)
#pragma unroll
  for (int c = 0; c < 12; ++c) k[c] = 0.0;
  k[0] = 200000.0;
  k[6] = 18000.0;
}

// A field of the handle's ResetDist block.  The block is uniform and no launch
// that reads it writes it (the setter is a launch of its own), so the kernels
// read it through the constant address space: scalar loads into SGPRs, issued
// only where an env resets.
template <class T>
SATENV_HD T rd_load(const T* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  return *(const __attribute__((address_space(4))) T*)p;
#else
  return *p;
#endif
}

// The randomised reset state of env i's episode `ep`:
// component c is lo[c] + span[c] * u with u = (w[c] + 0.5) * 2^-32 strictly
// inside (0, 1) and w the 12 words of three Philox4x32-10 blocks, counter
// (global env id, ep, block), key (seed, stream 2).  Integer rounds, an exact
// u and two f64 roundings (no contraction): the same bits on both targets.
// No rejection: a start inside d_capture is captured on its first step.
SATENV_HD void reset_draw(const ResetDist* d, int64_t i, uint32_t ep, double (&k)[12]) {
  const uint64_t gid = (uint64_t)rd_load(&d->env_offset) + (uint64_t)i;
  const uint32_t k0 = rd_load(&d->k0), k1 = rd_load(&d->k1);
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    uint32_t w[4] = {(uint32_t)gid, (uint32_t)(gid >> 32), ep, (uint32_t)j};
    philox4x32_10(w, k0, k1);
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const double u = ((double)w[m] + 0.5) * 0x1p-32;
      k[4 * j + m] = rd_load(&d->lo[4 * j + m]) + rd_load(&d->span[4 * j + m]) * u;
    }
  }
}

// The action agent g's thrusters execute for the commanded (clipped) action a
// of global env `gid` in step `cnt` of its episode `ep`:
//   a'[c] = clip16((float)(s * a[c] + e[c])),  s = 1 + mag * z[0],
//   e[c] = (dir * |a|) * z[1 + c],  z[m] = 2 * ((w[m] + 0.5) * 2^-32) - 1 in (-1, 1)
// with w one Philox4x32-10 block, counter (gid, ep, cnt), key (seed, stream 3 +
// g).  A magnitude error along the command plus an isotropic pointing error
// that scales with it: a zero command stays zero, and mag <= 1 keeps s > 0.
// Bounded uniforms on purpose: a Gaussian needs log / sincos, which are not
// the same bits on OCML and glibc, and the draw has to be (integer rounds, an
// exact u, then f64 products and sums each rounded once, no contraction; |a|
// is norm3's fma chain over exact squares of widened f32, so it is too).  An
// agent whose half-widths are both 0 draws nothing and keeps its bits.
SATENV_HD void act_noise(const ActNoise* d, int g, uint64_t gid, uint32_t ep, uint32_t cnt, float (&a)[3]) {
  const double mag = rd_load(&d->mag[g]), dir = rd_load(&d->dir[g]);
  if (mag == 0.0 && dir == 0.0) return;
  uint32_t w[4] = {(uint32_t)gid, (uint32_t)(gid >> 32), ep, cnt};
  philox4x32_10(w, rd_load(&d->k0[g]), rd_load(&d->k1[g]));
  double z[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) z[m] = 2.0 * (((double)w[m] + 0.5) * 0x1p-32) - 1.0;
  const double s = 1.0 + mag * z[0];
  const double r = dir * norm3((double)a[0], (double)a[1], (double)a[2]);
#pragma unroll
  for (int c = 0; c < 3; ++c) a[c] = clip16((float)(s * (double)a[c] + r * z[1 + c]));
}

// satenv_act_noise_host and its satenv_cpu_ twin: the model on host pointers;
// nullptr, or the refusal's reason
inline const char* act_noise_host(const satenv_act_noise* in, int64_t gid, int32_t ep, int32_t cnt, int32_t agent,
                                  const float* a_in, float* a_out) {
  if (!in || !a_in || !a_out) return "null argument";
  if (agent != 0 && agent != 1) return "agent must be 0 (pursuer) or 1 (evader)";
  ActNoise d;
  if (const char* bad = act_noise_pack(*in, d)) return bad;
  float a[3] = {a_in[0], a_in[1], a_in[2]};
  if (d.enabled) act_noise(&d, agent, (uint64_t)gid, (uint32_t)ep, (uint32_t)cnt, a);
  for (int c = 0; c < 3; ++c) a_out[c] = a[c];
  return nullptr;
}

// The measured kinematics m of the true k of global env `gid` at step `cnt` of
// its episode `ep`: scalar s of tracked craft g = s / 6 is
//   m[s] = k[s] + (B * z(wb[s]) + W * z(ww[s])),  z(w) = 2 * ((w + 0.5) * 2^-32) - 1
// with B the craft's bias half-width (bias_vel for a velocity scalar, s % 6 >=
// 3, else bias_pos), W its refreshed one (vel / pos), wb the 12 words of three
// Philox4x32-10 blocks, counter (gid, ep, j), key (seed, stream 5), and ww
// those of three blocks, counter (gid, ep, cnt / hold), key (seed, stream 6 +
// j).  A zero half-width leaves its product out (so m[s] is k[s] bit for bit
// where both are zero), and a block none of whose scalars has a non-zero
// half-width is not drawn.  Integer rounds, an exact u, f64 products and sums
// rounded once each: the same bits on both targets (as act_noise).  The half-
// widths are uniform, so every branch on them is a scalar one; the six chains
// are independent of each other and of the step, and unrolled side by side.
SATENV_HD void obs_measure(const ObsNoise* d, uint64_t gid, uint32_t ep, uint32_t cnt, const double (&k)[12],
                           double (&m)[12]) {
  double B[2][2], W[2][2];   // [craft][position / velocity]
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    B[g][0] = rd_load(&d->bias_pos[g]);
    B[g][1] = rd_load(&d->bias_vel[g]);
    W[g][0] = rd_load(&d->pos[g]);
    W[g][1] = rd_load(&d->vel[g]);
  }
  const bool has_b[2] = {B[0][0] != 0.0 || B[0][1] != 0.0, B[1][0] != 0.0 || B[1][1] != 0.0};
  const bool has_w[2] = {W[0][0] != 0.0 || W[0][1] != 0.0, W[1][0] != 0.0 || W[1][1] != 0.0};
  const uint32_t win = cnt / (uint32_t)rd_load(&d->hold);
  const uint32_t g0 = (uint32_t)gid, g1 = (uint32_t)(gid >> 32);
#pragma unroll
  for (int j = 0; j < 3; ++j) {   // block j: scalars 4j .. 4j + 3 (craft 0 in blocks 0, 1; craft 1 in 1, 2)
    uint32_t wb[4] = {g0, g1, ep, (uint32_t)j}, ww[4] = {g0, g1, ep, win};
    if ((j <= 1 && has_b[0]) || (j >= 1 && has_b[1])) philox4x32_10(wb, rd_load(&d->kb0), rd_load(&d->kb1));
    if ((j <= 1 && has_w[0]) || (j >= 1 && has_w[1])) philox4x32_10(ww, rd_load(&d->kw0[j]), rd_load(&d->kw1[j]));
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int s = 4 * j + q, g = s / 6, v = (s % 6) >= 3 ? 1 : 0;
      const double b = B[g][v], w = W[g][v];
      const double eb = b * (2.0 * (((double)wb[q] + 0.5) * 0x1p-32) - 1.0);
      const double ew = w * (2.0 * (((double)ww[q] + 0.5) * 0x1p-32) - 1.0);
      if (b != 0.0 && w != 0.0) m[s] = k[s] + (eb + ew);
      else if (b != 0.0) m[s] = k[s] + eb;
      else if (w != 0.0) m[s] = k[s] + ew;
      else m[s] = k[s];
    }
  }
}

// The f32 observation row of env i whose true kinematics are k, at (ep, cnt) of
// the rule in include/satenv.h: write_obs of the measured kinematics while the
// handle's observation noise is enabled, of the truth otherwise.  obs64 is the
// truth either way.
SATENV_HD void write_obs_measured(const ObsNoise* d, float* obs, double* obs64, int64_t i, uint32_t ep,
                                  uint32_t cnt, const double (&k)[12]) {
  if (obs != nullptr && rd_load(&d->enabled)) {
    double m[12];
    obs_measure(d, (uint64_t)rd_load(&d->env_offset) + (uint64_t)i, ep, cnt, k, m);
    write_obs(obs, nullptr, i, m);
    write_obs(nullptr, obs64, i, k);
  } else {
    write_obs(obs, obs64, i, k);
  }
}

// satenv_obs_noise_host and its satenv_cpu_ twin: the model on host pointers;
// nullptr, or the refusal's reason
inline const char* obs_noise_host(const satenv_obs_noise* in, int64_t gid, int32_t ep, int32_t cnt,
                                  const double* k_in, double* k_out, float* obs_out) {
  if (!in || !k_in || !k_out) return "null argument";
  ObsNoise d{};
  if (const char* bad = obs_noise_pack(*in, d)) return bad;
  double k[12], m[12];
  for (int c = 0; c < 12; ++c) m[c] = k[c] = k_in[c];
  if (d.enabled) obs_measure(&d, (uint64_t)gid, (uint32_t)ep, (uint32_t)cnt, k, m);
  for (int c = 0; c < 12; ++c) k_out[c] = m[c];
  if (obs_out) {
    alignas(8) float row[18];
    write_obs(row, nullptr, 0, m);
    for (int c = 0; c < 18; ++c) obs_out[c] = row[c];
  }
  return nullptr;
}

// One reset of env i (the masked reset and the autoreset): the kinematics it
// starts from and its vel_int bit -- the reference's int64 constants (vel_int
// 1) or, with the distribution enabled, the draw of this episode index (float
// velocities, vel_int 0: no first-step truncation).  Every reset advances
// the env's episode index.  kDraw = false: the instantiation of handles that
// never enabled a distribution, without the draw's code (as kRk45 below).
template <bool kDraw>
SATENV_HD int reset_state(const Params& prm, const ResetDist* rd, int64_t n, int32_t* i32, int64_t i,
                          double (&k)[12]) {
  const int32_t ep = i32[kPlaneEp * n + i];
  i32[kPlaneEp * n + i] = ep + 1;
  if constexpr (kDraw) {
    if (rd_load(&rd->enabled)) {
      reset_draw(rd, i, (uint32_t)ep, k);
      return 0;
    }
  }
  reset_kin(prm, k);
  return 1;
}

// env i as the constructor leaves it (environment.py:26-44)
SATENV_HD void init_env(const Params& p, int64_t n, double* f64, int32_t* i32, int64_t i) {
#pragma unroll
  for (int c = 0; c < 12; ++c) f64[c * n + i] = p.init_kin[c];              // :30-33
  f64[12 * n + i] = p.fuel_c0;                                              // :42-43
  f64[13 * n + i] = p.fuel_t0;
  f64[14 * n + i] = INFINITY;                                               // :44
  f64[kPlaneRet * n + i] = 0.0;
  i32[kPlaneDz * n + i] = 0;                                                // :41
  i32[kPlaneCount * n + i] = 0;
  i32[kPlaneBits * n + i] = make_bits(p.fuel_c0_mode, p.fuel_t0_mode, 1, p.flag);
  i32[kPlaneEp * n + i] = 0;
}

// reset(Flag) of env i where the mask selects it (environment.py:66-79), and its obs either way
// kMeas: the row is measured under the handle's observation noise `on` (the
// reset kernel of handles that enabled it once, and the host build)
template <bool kMeas = false>
SATENV_HD void reset_env(const Params& prm, const ResetDist* rd, int64_t n, double* f64, int32_t* i32, int32_t flag,
                         const uint8_t* mask, float* obs, double* obs64, int64_t i, const ObsNoise* on = nullptr) {
  double k[12];
  if (mask == nullptr || mask[i] != 0) {
    const int vi = reset_state<true>(prm, rd, n, i32, i, k);
#pragma unroll
    for (int c = 0; c < 12; ++c) f64[c * n + i] = k[c];
    const int b = i32[kPlaneBits * n + i];
    i32[kPlaneBits * n + i] = make_bits(fc_mode(b), ft_mode(b), vi, flag);
    i32[kPlaneCount * n + i] = 0;
    f64[kPlaneRet * n + i] = 0.0;
  } else {
#pragma unroll
    for (int c = 0; c < 12; ++c) k[c] = f64[c * n + i];
  }
  if constexpr (kMeas)   // a reset env: its advanced index and count 0; the others: their planes as they are
    write_obs_measured(on, obs, obs64, i, (uint32_t)i32[kPlaneEp * n + i], (uint32_t)i32[kPlaneCount * n + i], k);
  else
    write_obs(obs, obs64, i, k);
}

// ---------------------------------------------------------------------------
// One environment step (environment.py:81-255), one lane per env, in two
// halves around the danger-zone count: step_begin (actions, fuel, STM,
// terminal tests, the count's set-up) and step_end (count, reward, outputs,
// autoreset, state write-back).
// ---------------------------------------------------------------------------
struct Lane {
  double k[12];
  double fuel_c, fuel_t, dis, dis_prev;
  int dz, count, flag, fcm, ftm;
  bool p_zero;
  float pa[3];
  int err;                // propagator 2: scipy's TOO_SMALL_STEP (-6), else 0
  bool terminal;          // reward/done final, no count: capture or timeout (:139-147 return first), or Flag 2
  double reward;
  bool done;
};

// kRk45: the instantiation that carries propagator 2 (solve_ivp RK45); the
// default kernels leave it out so its registers do not cost the STM path
// occupancy.  kNoise: the instantiation of handles that enabled actuation
// noise once; the others do not carry its code (as kDraw in reset_state).
template <bool kRk45 = false, bool kNoise = false>
SATENV_HD void step_begin(const Params& prm, int64_t n, const double* __restrict__ f64,
                                           const int32_t* __restrict__ i32, const StepIO& io, int64_t i,
                                           bool autoreset, Lane& L, StepStats& s) {
  double* k = L.k;
#pragma unroll
  for (int c = 0; c < 12; ++c) k[c] = f64[c * n + i];
  L.fuel_c = f64[12 * n + i];
  L.fuel_t = f64[13 * n + i];
  L.dis = f64[14 * n + i];
  L.dz = i32[kPlaneDz * n + i];
  const int bits = i32[kPlaneBits * n + i];
  if (autoreset || io.ext_count == nullptr) L.count = i32[kPlaneCount * n + i] + 1;
  else L.count = io.ext_count[i];
  L.flag = env_flag(bits);
  const int vi = vel_int(bits);
  L.fcm = fc_mode(bits);
  L.ftm = ft_mode(bits);
  float ea[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    L.pa[c] = clip16(io.pa[i * 3 + c]);                                  // :86-87
    ea[c] = clip16(io.ea[i * 3 + c]);
  }
  if constexpr (kNoise) {                                                 // from here on the env sees the
    if (rd_load(&io.an->enabled)) {                                       // executed actions only
      const uint64_t gid = (uint64_t)rd_load(&io.an->env_offset) + (uint64_t)i;
      const uint32_t ep = (uint32_t)i32[kPlaneEp * n + i];
      act_noise(io.an, 0, gid, ep, (uint32_t)L.count, L.pa);
      act_noise(io.an, 1, gid, ep, (uint32_t)L.count, ea);
    }
  }
  L.dis_prev = norm3(k[0] - k[6], k[1] - k[7], k[2] - k[8]);             // :89
  bool p_zero = false, e_zero = false, move_p = true, move_e = true;
  if (L.flag != 1) {                                                      // Flag 0 and Flag 2 (:262-276)
    if (L.dis < prm.d_range && L.dz != 0) { move_p = false; p_zero = true; }   // :91-97
  } else {
    if (L.dz == 0) { move_e = false; e_zero = true; }                         // :194-198
  }
  L.p_zero = p_zero;
#pragma unroll
  for (int c = 0; c < 3; ++c) {                                           // Vector[i] += action[i]
    if (move_p) { const double t = k[3 + c] + (double)L.pa[c]; k[3 + c] = vi ? trunc(t) : t; }
    if (move_e) { const double t = k[9 + c] + (double)ea[c]; k[9 + c] = vi ? trunc(t) : t; }
  }
  fuel_sub(L.fuel_c, L.fcm, p_zero, (fabsf(L.pa[0]) + fabsf(L.pa[1])) + fabsf(L.pa[2]));   // :106
  fuel_sub(L.fuel_t, L.ftm, e_zero, (fabsf(ea[0]) + fabsf(ea[1])) + fabsf(ea[2]));         // :107

  L.err = 0;
  bool propagated = false;
  if constexpr (kRk45) {
    if (prm.propagator == 2) {                                            // optional: solve_ivp RK45 (:783-839)
#pragma unroll 1
      for (int craft = 0; craft < 2; ++craft) {
        double x[6];
#pragma unroll
        for (int c = 0; c < 6; ++c) x[c] = k[6 * craft + c];
        const int rc = cw_rk45(x, 100.0);
        if (rc) L.err = rc;
#pragma unroll
        for (int c = 0; c < 6; ++c) k[6 * craft + c] = x[c];
      }
      propagated = true;
    }
  }
  if (propagated) {
  } else if (prm.propagator == 1) {                                       // optional: RK4 on the CW ODE
#pragma unroll
    for (int craft = 0; craft < 2; ++craft) {
      double x[6];
#pragma unroll
      for (int c = 0; c < 6; ++c) x[c] = k[6 * craft + c];
      cw_rk4(x, prm.cw_omega, 100.0, prm.rk4_substeps);
#pragma unroll
      for (int c = 0; c < 6; ++c) k[6 * craft + c] = x[c];
    }
  } else {
    // Clohessy-Wiltshire STM (satellite_function.py:776-779), OpenBLAS dgemv_t order
    double y[12];
#pragma unroll
    for (int craft = 0; craft < 2; ++craft) {
      const double* x = k + 6 * craft;
#pragma unroll
      for (int r = 0; r < 6; ++r) {
        const double* M = prm.stm + 6 * r;
        const double p0 = M[0] * x[0], p1 = M[1] * x[1], p2 = M[2] * x[2];
        const double p3 = M[3] * x[3], p4 = M[4] * x[4], p5 = M[5] * x[5];
        y[6 * craft + r] = (((p0 + p2) + (p1 + p3)) + p4) + p5;
      }
    }
#pragma unroll
    for (int c = 0; c < 12; ++c) k[c] = y[c];
  }
  L.dis = norm3(k[0] - k[6], k[1] - k[7], k[2] - k[8]);                   // :132
  L.terminal = true;
  L.done = true;
  if (L.dis <= prm.d_capture) {                                           // :139-142, :221-225, :303-306
    L.reward = L.flag == 0 ? prm.win_reward : (L.flag == 1 ? -150.0 : 0.0);
    s.cap = 1.0;
  } else if (L.count >= prm.max_episode_steps) {                         // :144-147, :227-231, :308-311
    L.reward = L.flag == 0 ? prm.burn_reward : (L.flag == 1 ? prm.win_reward : 0.0);
  } else if (L.flag == 2) {                                               // :313-315: reward 0, not done,
    L.reward = 0.0;                                                       // no danger-zone update (the
    L.done = false;                                                       // ellipse fit and the surrogate
  } else {                                                                // training run outside the kernel)
    L.terminal = false;
    L.done = false;
  }
}

// the count-independent reward terms 1*pv1, 0.6*pv2, 0.2*pv3, 2*pv4 (:166-175)
SATENV_HD void reward_terms(const double (&k)[12], const float (&pa)[3], bool p_zero, double (&t)[4]) {
  const double r0 = k[0] - k[6], r1 = k[1] - k[7], r2 = k[2] - k[8];
  const double pv1 = cos_sim(k[0], k[1], k[2], k[6], k[7], k[8]);       // reward_of_action3
  const double pv2 = cos_sim(k[3], k[4], k[5], k[9], k[10], k[11]);     // reward_of_action1
  const double pv3 = cos_sim(r0, r1, r2, k[3], k[4], k[5]);             // reward_of_action2
  double pv4 = 0.0;                                                      // reward_of_action4, :388
  if (!p_zero && pa[0] != 0.0f && pa[1] != 0.0f && pa[2] != 0.0f) {
    const double nr = norm3(r0, r1, r2);
    const float na = norm3f(pa[0], pa[1], pa[2]);
    pv4 = -dot3(r0 / nr, r1 / nr, r2 / nr, (double)(pa[0] / na), (double)(pa[1] / na), (double)(pa[2] / na));
  }
  t[0] = 1 * pv1;
  t[1] = 0.6 * pv2;
  t[2] = 0.2 * pv3;
  t[3] = 2 * pv4;
}

// non-terminal reward with the new danger-zone count (:150, :161-175, :251)
SATENV_HD void step_reward_terms(const Params& prm, Lane& L, int cnt, const double (&t)[4]) {
  L.dz = cnt;
  double r = (L.dis < L.dis_prev) ? 1.0 : -1.0;                          // :161-164
  r += (prm.d_capture <= L.dis && L.dis <= 4 * prm.d_capture) ? -1.0 : -2.0;
  r += (L.dz == 0) ? -1.0 : L.dz * 0.5;
  r += t[0];
  r += t[1];
  r += t[2];
  r += t[3];
  L.reward = L.flag == 0 ? r : -r;                                        // :251
}

SATENV_HD void step_reward(const Params& prm, Lane& L, int cnt) {
  double t[4];
  reward_terms(L.k, L.pa, L.p_zero, t);
  step_reward_terms(prm, L, cnt, t);
}

// kMeas: the instantiation of handles that enabled observation noise once
// (the f32 row is write_obs_measured's); the others do not carry its code.
template <bool kDraw = false, bool kMeas = false>
SATENV_HD void step_end(const Params& prm, int64_t n, double* __restrict__ f64,
                                         int32_t* __restrict__ i32, const StepIO& io, int64_t i, bool autoreset,
                                         Lane& L, StepStats& s) {
  if (io.rew64) io.rew64[i] = L.reward;
  if (io.rew32) io.rew32[i] = (float)L.reward;
  if (io.done) io.done[i] = L.done ? 1 : 0;
  double ret = f64[kPlaneRet * n + i] + L.reward;
  s.rew = L.reward;
  int vi_out = 0;
  if (autoreset && L.done) {                                              // CPPO_main.py:149-153 -> reset(Flag)
    s.fin = 1.0;
    s.fin_ret = ret;
    ret = 0.0;
    vi_out = reset_state<kDraw>(prm, io.rd, n, i32, i, L.k);
    L.count = 0;
  }
  if constexpr (kMeas)   // the episode index after this launch, the count this step used (0 after the autoreset)
    write_obs_measured(io.on, io.obs, io.obs64, i, (uint32_t)i32[kPlaneEp * n + i], (uint32_t)L.count, L.k);
  else
    write_obs(io.obs, io.obs64, i, L.k);
#pragma unroll
  for (int c = 0; c < 12; ++c) f64[c * n + i] = L.k[c];
  f64[12 * n + i] = L.fuel_c;
  f64[13 * n + i] = L.fuel_t;
  f64[14 * n + i] = L.dis;
  f64[kPlaneRet * n + i] = ret;
  i32[kPlaneDz * n + i] = L.dz;
  i32[kPlaneCount * n + i] = L.count;
  i32[kPlaneBits * n + i] = make_bits(L.fcm, L.ftm, vi_out, L.flag);
}

// The whole step of env i in one lane (the count's four solves one after
// another): the one-lane kernel and the host build.  Returns the error code
// to record, 0 if none; the caller owns the (first-wins) error sink.
template <bool kRk45, bool kDraw, bool kNoise = false, bool kMeas = false>
SATENV_HD int step_lane(const Params& prm, int64_t n, double* __restrict__ f64, int32_t* __restrict__ i32,
                        const StepIO& io, int64_t i, bool autoreset, StepStats& s) {
  Lane L;
  step_begin<kRk45, kNoise>(prm, n, f64, i32, io, i, autoreset, L, s);
  int err = L.err;
  if (!L.terminal) {
    int cnt = 0;
    const int rc = danger_zone(prm, L.k, L.fuel_c, L.fcm, cnt);            // :150, :317-332
    if (err == 0) err = rc;
    step_reward(prm, L, cnt);
  }
  step_end<kDraw, kMeas>(prm, n, f64, i32, io, i, autoreset, L, s);
  return err;
}

}  // namespace satenv
