// rollout_kernels.hip -- gfx950 kernels behind include/satrl_rollout.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "philox_device.h"
#include "satrl_error.h"
#include "satrl_rollout.h"

namespace {

// ---------------------------------------------------------------------------
// GAE reverse scan (ppo_continuous.py:201-208), one lane per env.  The time
// loop is sequential per env; loads of steps t-1.. are independent of the
// carried gae, so the unrolled loop keeps several rows in flight per lane.
// f32, reference operation order, compiled with -ffp-contract=off.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) gae_kernel(int64_t T, int64_t N, const float* __restrict__ r,
                                                  const uint8_t* __restrict__ done, const float* __restrict__ v,
                                                  float gamma, float c, float* __restrict__ adv,
                                                  float* __restrict__ vt) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  float gae = 0.0f;
  float v_next = v[T * N + i];
#pragma unroll 8
  for (int64_t t = T - 1; t >= 0; --t) {
    const int64_t o = t * N + i;
    const float v_t = v[o];
    const float dw = (float)done[o];
    const float delta = (r[o] + (gamma * (1.0f - dw)) * v_next) - v_t;   // r + g*(1-dw)*vs_ - vs
    gae = delta + (c * gae) * (1.0f - dw);                               // delta + g*l*gae*(1-d)
    adv[o] = gae;
    vt[o] = gae + v_t;                                                    // v_target = adv + vs
    v_next = v_t;
  }
}

// League tally (satrl_league_tally): finished episodes and captures of a
// rollout per 32-env block.  One lane per env scans T in gae_kernel's shape
// (coalesced across envs, the unrolled loop keeps several rows in flight);
// lanes past N count nothing and stay for the reduction.  A block is one half
// of a wave: five xor shuffles below 32 add its lanes, and the half's first
// lane adds to the block's two words -- integers, no atomics, no order.
__global__ void __launch_bounds__(64) league_tally_kernel(int64_t T, int64_t N, const float* __restrict__ rew,
                                                          const uint8_t* __restrict__ done, float capture_reward,
                                                          int64_t* __restrict__ tally) {
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  int ep = 0, cap = 0;                                            // (T * 1 per lane: the host refuses T above 2^31 - 1)
  if (i < N) {
#pragma unroll 8
    for (int64_t t = 0; t < T; ++t) {
      const int64_t o = t * N + i;
      const int d = done[o] != 0;
      ep += d;
      cap += d & (int)(rew[o] == capture_reward);
    }
  }
#pragma unroll
  for (int off = 16; off > 0; off >>= 1) {
    ep += __shfl_xor(ep, off, 64);
    cap += __shfl_xor(cap, off, 64);
  }
  if ((threadIdx.x & 31) == 0 && i < N) {
    int64_t* w = tally + (i >> 5) * 2;
    w[0] += ep;
    w[1] += cap;
  }
}

// choose_action (ppo_continuous.py:184-188): a = clamp(mean + std*z, +-max);
// log_prob(a) per dim as torch.distributions.Normal.log_prob.  Noise:
// philox_device.h, keyed by (seed, agent, global env id, step).
__global__ void __launch_bounds__(256) gaussian_kernel(int64_t N, const float* __restrict__ mean,
                                                       const float* __restrict__ log_std, float max_action,
                                                       uint32_t k0, uint32_t k1, int64_t env_offset,
                                                       uint64_t step, const uint64_t* __restrict__ step_base,
                                                       float* __restrict__ act,
                                                       float* __restrict__ logp) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  if (step_base) step += *step_base;
  float z[4];
  philox_normal4((uint64_t)(env_offset + i), step, k0, k1, z);
#pragma unroll
  for (int d = 0; d < 3; ++d) gaussian_act(mean[i * 3 + d], log_std[d], z[d], max_action, act[i * 3 + d], logp[i * 3 + d]);
}

__global__ void __launch_bounds__(256) moments_kernel(int64_t n, const float* __restrict__ x,
                                                      double* __restrict__ out) {
  double s = 0.0, s2 = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const double v = x[i];
    s += v;
    s2 += v * v;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    s += __shfl_xor(s, off, 64);
    s2 += __shfl_xor(s2, off, 64);
  }
  __shared__ double red[2][4];
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { red[0][w] = s; red[1][w] = s2; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = 0.0, b = 0.0;
    for (int k = 0; k < (int)(blockDim.x >> 6); ++k) { a += red[0][k]; b += red[1][k]; }
    atomicAdd(out, a);
    atomicAdd(out + 1, b);
  }
}

// The same sums with a fixed order of additions (satrl_moments_ordered): the
// blocks of moments_partial_kernel leave their sums in part[2][blocks], and one
// block of moments_combine_kernel adds those in block order, so the result
// does not depend on which block finishes first (the atomics above do).
__device__ __forceinline__ void block_sum2(double& s, double& s2) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    s += __shfl_xor(s, off, 64);
    s2 += __shfl_xor(s2, off, 64);
  }
  __shared__ double red[2][4];
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { red[0][w] = s; red[1][w] = s2; }
  __syncthreads();
  s = 0.0;
  s2 = 0.0;
  for (int k = 0; k < (int)(blockDim.x >> 6); ++k) { s += red[0][k]; s2 += red[1][k]; }
}

__global__ void __launch_bounds__(256) moments_partial_kernel(int64_t n, const float* __restrict__ x,
                                                              double* __restrict__ part) {
  double s = 0.0, s2 = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const double v = x[i];
    s += v;
    s2 += v * v;
  }
  block_sum2(s, s2);
  if (threadIdx.x == 0) {
    part[blockIdx.x] = s;
    part[gridDim.x + blockIdx.x] = s2;
  }
}

__global__ void __launch_bounds__(256) moments_combine_kernel(int blocks, const double* __restrict__ part,
                                                              double* __restrict__ out) {
  double s = 0.0, s2 = 0.0;
  for (int k = threadIdx.x; k < blocks; k += blockDim.x) {
    s += part[k];
    s2 += part[blocks + k];
  }
  block_sum2(s, s2);
  if (threadIdx.x == 0) {
    out[0] += s;
    out[1] += s2;
  }
}

// ---------------------------------------------------------------------------
// Running observation normalisation (normalization.py:38-47 with frozen
// statistics): out = clamp((raw - mean) * inv_std, +-clip), one subtract and
// one multiply in f32.  One wave per 32-env slot: the slot's 576 floats are
// 144 16-byte lane loads (three per lane, the third on lanes 0..15).
//
// Accumulators (acc != NULL): the slot's raw rows are staged in LDS; lane
// f + 18 h (f < 18, h < 2) sums d = (double)raw - (double)pivot[f] and d*d
// over rows 16 h .. 16 h + 15 in row order, the two halves are added (low +
// high) and the slot's owner lane adds the total to acc[slot] with a plain
// read-modify-write.  The order depends on the row's index in the slot only,
// so the sums are bitwise reproducible and a shard that starts at a multiple
// of 32 envs writes the unsharded run's slots.
// ---------------------------------------------------------------------------
constexpr int kObsDim = 18;
constexpr int kSlotRows = 32;
constexpr int kSlotFloats = kSlotRows * kObsDim;   // 576
constexpr int kSlotVec4 = kSlotFloats / 4;         // 144

__device__ __forceinline__ float clamp_keep_nan(float x, float c) { return x < -c ? -c : (x > c ? c : x); }

__global__ void __launch_bounds__(64) obs_normalize_kernel(int64_t N, const float* __restrict__ raw,
                                                           const float* __restrict__ stats, float clip,
                                                           float* __restrict__ out, const float* __restrict__ pivot,
                                                           double* __restrict__ acc, int vec) {
  __shared__ float s_stats[2 * kObsDim];
  __shared__ float s_pivot[kObsDim];
  __shared__ __attribute__((aligned(16))) float s_raw[kSlotFloats];
  const int lane = threadIdx.x;
  const int64_t slot = blockIdx.x;
  const int64_t base = slot * kSlotFloats;          // first float of the slot
  const int64_t lim = N * kObsDim;                  // one past the last float of raw / out
  // every global load of the launch is issued before the first wait: the statistics, the
  // lane's pieces of the slot and the owner lanes' accumulator words
  const float sv = lane < 2 * kObsDim ? stats[lane] : 0.0f;
  const float pv = acc && lane < kObsDim ? pivot[lane] : 0.0f;
  double* const a = acc ? acc + slot * (2 * kObsDim) : nullptr;
  double a0 = 0.0, a1 = 0.0;
  if (acc && lane < kObsDim) { a0 = a[lane]; a1 = a[kObsDim + lane]; }
  float x[3][4];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int j = lane + 64 * k;                    // the lane's k-th 16-byte piece of the slot
    const int64_t e = base + 4 * j;
#pragma unroll
    for (int c = 0; c < 4; ++c) x[k][c] = 0.0f;
    if (j >= kSlotVec4 || e >= lim) continue;
    if (vec && e + 4 <= lim) {
      const float4 v = *reinterpret_cast<const float4*>(raw + e);
      x[k][0] = v.x; x[k][1] = v.y; x[k][2] = v.z; x[k][3] = v.w;
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (e + c < lim) x[k][c] = raw[e + c];
    }
  }
  if (lane < 2 * kObsDim) s_stats[lane] = sv;
  if (lane < kObsDim) s_pivot[lane] = pv;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int j = lane + 64 * k;
    if (acc && j < kSlotVec4) *reinterpret_cast<float4*>(s_raw + 4 * j) = make_float4(x[k][0], x[k][1], x[k][2], x[k][3]);
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int j = lane + 64 * k;
    const int64_t e = base + 4 * j;
    if (j >= kSlotVec4 || e >= lim) continue;
    float y[4];
    int f = (4 * j) % kObsDim;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float z = (x[k][c] - s_stats[f]) * s_stats[kObsDim + f];
      y[c] = clip > 0.0f ? clamp_keep_nan(z, clip) : z;
      f = f + 1 == kObsDim ? 0 : f + 1;
    }
    if (vec && e + 4 <= lim) {
      *reinterpret_cast<float4*>(out + e) = make_float4(y[0], y[1], y[2], y[3]);
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (e + c < lim) out[e + c] = y[c];
    }
  }
  if (!acc) return;                                  // (uniform: a kernel argument)
  const int64_t left = N - slot * kSlotRows;
  const int rows = left < kSlotRows ? (int)left : kSlotRows;
  const int f = lane % kObsDim, h = lane / kObsDim;  // lanes 36.. idle (h >= 2): they re-read half 0
  const int r0 = h < 2 ? 16 * h : 0;
  const double p = (double)s_pivot[f];
  float v[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) v[q] = s_raw[(r0 + q) * kObsDim + f];   // the 16 LDS reads in flight together
  double s = 0.0, s2 = 0.0;
#pragma unroll
  for (int q = 0; q < 16; ++q) {                     // row order; a row past N adds +0.0, which is exact
    const double d = r0 + q < rows ? (double)v[q] - p : 0.0;
    s += d;
    s2 += d * d;
  }
  const double hs = __shfl_down(s, kObsDim, 64);     // lane f takes rows 16..31 from lane f + 18
  const double hs2 = __shfl_down(s2, kObsDim, 64);
  if (lane < kObsDim) {
    a[lane] = a0 + (s + hs);
    a[kObsDim + lane] = a1 + (s2 + hs2);
  }
}

// ---------------------------------------------------------------------------
// Discounted-return scan of RewardScaling (normalization.py:50-63): one lane
// per env, forward over t, R = gamma * R + r in f64 (no FMA); the lane sums R
// and R * R over t in registers, R = 0 after a done step.  A slot's 32 lanes
// are then combined by an xor butterfly (16, 8, 4, 2, 1; a + b == b + a, so
// the pairing depends on the lane's index in the slot only) and lane 0 of the
// slot adds the totals to acc[slot] with a plain read-modify-write.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(64) return_scan_kernel(int64_t T, int64_t N, const float* __restrict__ r,
                                                         const uint8_t* __restrict__ done, double gamma,
                                                         double* __restrict__ carry, double* __restrict__ acc) {
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  const bool live = i < N;
  const int64_t ii = live ? i : N - 1;               // idle lanes re-read the last env and contribute nothing
  double R = carry[ii];
  double s = 0.0, s2 = 0.0;
#pragma unroll 8
  for (int64_t t = 0; t < T; ++t) {
    const int64_t o = t * N + ii;
    R = gamma * R + (double)r[o];
    s += R;
    s2 += R * R;
    if (done[o]) R = 0.0;
  }
  if (live) carry[i] = R;
  else { s = 0.0; s2 = 0.0; }
#pragma unroll
  for (int off = 16; off > 0; off >>= 1) {
    s += __shfl_xor(s, off, 64);
    s2 += __shfl_xor(s2, off, 64);
  }
  if (live && (threadIdx.x & 31) == 0) {
    double* a = acc + (i >> 5) * 2;
    a[0] += s;
    a[1] += s2;
  }
}

// ---------------------------------------------------------------------------
// Episode records of an evaluation (one lane per env, SoA planes): the first
// episode of every env is summed in f64 in step order and frozen at its done
// step.  rec_f64 planes: ret, final_dis, min_dis, dv_p, dv_e; rec_i32 planes:
// length, outcome (0 running, 1 captured, 2 timed out).  *alive counts the
// envs still running: a wave's newly finished envs are counted by a ballot
// and taken off by one vector atomic of its first lane.
// ---------------------------------------------------------------------------
constexpr int kRecRet = 0, kRecFinalDis = 1, kRecMinDis = 2, kRecDvP = 3, kRecDvE = 4;
constexpr int kRecLength = 0, kRecOutcome = 1;

__global__ void __launch_bounds__(64) episode_record_reset_kernel(int64_t N, double* __restrict__ rf,
                                                                  int32_t* __restrict__ ri,
                                                                  int32_t* __restrict__ alive) {
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (i == 0) *alive = (int32_t)N;
  if (i >= N) return;
  rf[kRecRet * N + i] = 0.0;
  rf[kRecFinalDis * N + i] = __builtin_nan("");
  rf[kRecMinDis * N + i] = __builtin_inf();
  rf[kRecDvP * N + i] = 0.0;
  rf[kRecDvE * N + i] = 0.0;
  ri[kRecLength * N + i] = 0;
  ri[kRecOutcome * N + i] = 0;
}

__device__ __forceinline__ double abs_sum3(const float* __restrict__ a) {
  return (fabs((double)a[0]) + fabs((double)a[1])) + fabs((double)a[2]);
}

__global__ void __launch_bounds__(64) episode_record_kernel(int64_t N, const double* __restrict__ reward,
                                                            const uint8_t* __restrict__ done,
                                                            const double* __restrict__ obs64,
                                                            const float* __restrict__ pa, const float* __restrict__ ea,
                                                            double capture_reward, double* __restrict__ rf,
                                                            int32_t* __restrict__ ri, int32_t* __restrict__ alive) {
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  bool finished = false;
  if (i < N && ri[kRecOutcome * N + i] == 0) {
    const double r = reward[i];
    const double* o = obs64 + i * kObsDim;
    const double dis = sqrt((o[0] * o[0] + o[1] * o[1]) + o[2] * o[2]);
    rf[kRecRet * N + i] += r;
    rf[kRecDvP * N + i] += abs_sum3(pa + i * 3);
    rf[kRecDvE * N + i] += abs_sum3(ea + i * 3);
    ri[kRecLength * N + i] += 1;
    if (dis < rf[kRecMinDis * N + i]) rf[kRecMinDis * N + i] = dis;
    if (done[i]) {
      rf[kRecFinalDis * N + i] = dis;
      ri[kRecOutcome * N + i] = r == capture_reward ? 1 : 2;
      finished = true;
    }
  }
  const unsigned long long m = __ballot(finished);               // (every lane of the wave is here)
  if (m != 0ull && threadIdx.x == 0) atomicSub(alive, (int32_t)__popcll(m));
}

using satrl_err::fail;
using satrl_err::launch;
using satrl_err::null_arg;

// an entry point's count (T or N) under its own name
int positive(const char* who, const char* name, int64_t n) {
  return n > 0 ? 0 : fail(-1, who, std::string(name) + " must be positive");
}
// the 2 x blocks doubles of satrl_moments_ordered's scratch
int64_t moments_scratch(const char* who, int64_t n) {
  if (positive(who, "n", n)) return -1;
  return 2 * std::min<int64_t>((n + 255) / 256, 1024);
}

}  // namespace

extern "C" {

int satrl_obs_normalize(int64_t N, const float* raw, const float* stats, float clip, float* out, const float* pivot,
                        double* acc, void* stream) {
  if (int rc = positive(__func__, "N", N)) return rc;
  if (int rc = null_arg(__func__, SATRL_PTRS(raw, stats, out))) return rc;
  if (raw == out) return fail(-1, __func__, "out must not be raw");
  if (acc && !pivot) return fail(-1, __func__, "pivot is NULL with a non-NULL acc");
  const int64_t slots = (N + kSlotRows - 1) / kSlotRows;
  // 16-byte lane accesses need both row buffers on a 16-byte boundary (a slot is 2304 bytes)
  const int vec = (((uintptr_t)raw | (uintptr_t)out) & 15) == 0;
  return launch(__func__, obs_normalize_kernel, slots, 64, stream, N, raw, stats, clip, out, pivot, acc, vec);
}

int satrl_return_scan(int64_t T, int64_t N, const float* r, const uint8_t* done, double gamma, double* carry,
                      double* acc, void* stream) {
  if (int rc = positive(__func__, "T", T)) return rc;
  if (int rc = positive(__func__, "N", N)) return rc;
  if (int rc = null_arg(__func__, SATRL_PTRS(r, done, carry, acc))) return rc;
  return launch(__func__, return_scan_kernel, (N + 63) / 64, 64, stream, T, N, r, done, gamma, carry, acc);
}

int satrl_episode_record_reset(int64_t N, double* rec_f64, int32_t* rec_i32, int32_t* alive, void* stream) {
  if (int rc = positive(__func__, "N", N)) return rc;
  if (N > INT32_MAX) return fail(-1, __func__, "*alive is an int32");
  if (int rc = null_arg(__func__, SATRL_PTRS(rec_f64, rec_i32, alive))) return rc;
  return launch(__func__, episode_record_reset_kernel, (N + 63) / 64, 64, stream, N, rec_f64, rec_i32, alive);
}

int satrl_episode_record(int64_t N, const double* reward, const uint8_t* done, const double* obs64, const float* pa,
                         const float* ea, double capture_reward, double* rec_f64, int32_t* rec_i32, int32_t* alive,
                         void* stream) {
  if (int rc = positive(__func__, "N", N)) return rc;
  if (int rc = null_arg(__func__, SATRL_PTRS(reward, done, obs64, pa, ea, rec_f64, rec_i32, alive))) return rc;
  return launch(__func__, episode_record_kernel, (N + 63) / 64, 64, stream, N, reward, done, obs64, pa, ea,
                capture_reward, rec_f64, rec_i32, alive);
}

int satrl_gae(int64_t T, int64_t N, const float* r, const uint8_t* done, const float* v, float gamma, float lamda,
              float* adv_out, float* vtarget_out, void* stream) {
  if (int rc = positive(__func__, "T", T)) return rc;
  if (int rc = positive(__func__, "N", N)) return rc;
  if (int rc = null_arg(__func__, SATRL_PTRS(r, done, v, adv_out, vtarget_out))) return rc;
  // gamma*lamda is a python float product, rounded to f32 when it meets the
  // np.float32 gae (NEP 50), ppo_continuous.py:205
  const float c = (float)((double)gamma * (double)lamda);
  const int block = 64;   // N = 16384 envs -> 256 single-wave workgroups, one per CU
  return launch(__func__, gae_kernel, (N + block - 1) / block, block, stream, T, N, r, done, v, gamma, c, adv_out,
                vtarget_out);
}

int satrl_league_tally(int64_t T, int64_t N, const float* rew, const uint8_t* done, float capture_reward,
                       int64_t* tally, void* stream) {
  if (int rc = positive(__func__, "T", T)) return rc;
  if (int rc = positive(__func__, "N", N)) return rc;
  if (T > INT32_MAX) return fail(-1, __func__, "T is above what a lane's 32-bit count holds");
  if (int rc = null_arg(__func__, SATRL_PTRS(rew, done, tally))) return rc;
  return launch(__func__, league_tally_kernel, (N + 63) / 64, 64, stream, T, N, rew, done, capture_reward, tally);
}

int satrl_gaussian_sample(int64_t N, const float* mean, const float* log_std, float max_action, uint64_t seed,
                          uint32_t agent, int64_t env_offset, uint64_t step, const uint64_t* step_base,
                          float* act_out, float* logp_out, void* stream) {
  if (int rc = positive(__func__, "N", N)) return rc;
  if (int rc = null_arg(__func__, SATRL_PTRS(mean, log_std, act_out, logp_out))) return rc;
  uint32_t k0, k1;
  philox_key(seed, agent, k0, k1);
  return launch(__func__, gaussian_kernel, (N + 255) / 256, 256, stream, N, mean, log_std, max_action, k0, k1,
                env_offset, step, step_base, act_out, logp_out);
}

int satrl_moments(int64_t n, const float* x, double* out, void* stream) {
  if (int rc = positive(__func__, "n", n)) return rc;
  if (int rc = null_arg(__func__, SATRL_PTRS(x, out))) return rc;
  int64_t blocks = (n + 255) / 256;
  if (blocks > 1024) blocks = 1024;
  return launch(__func__, moments_kernel, blocks, 256, stream, n, x, out);
}

int64_t satrl_moments_scratch(int64_t n) { return moments_scratch(__func__, n); }

int satrl_moments_ordered(int64_t n, const float* x, double* out, double* scratch, int64_t scratch_elems,
                          void* stream) {
  const int64_t need = moments_scratch(__func__, n);
  if (need < 0) return -1;
  if (int rc = null_arg(__func__, SATRL_PTRS(x, out, scratch))) return rc;
  if (scratch_elems < need)
    return fail(-1, __func__, "scratch holds " + std::to_string(scratch_elems) + " doubles, " + std::to_string(need) +
                             " are needed");
  const int blocks = (int)(need / 2);
  if (int rc = launch(__func__, moments_partial_kernel, blocks, 256, stream, n, x, scratch)) return rc;
  return launch(__func__, moments_combine_kernel, 1, 256, stream, blocks, scratch, out);
}

const char* satrl_last_error(void) { return satrl_err::slot.c_str(); }

}  // extern "C"
