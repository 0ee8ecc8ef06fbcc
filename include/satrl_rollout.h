/*
 * satrl_rollout.h -- C ABI of the rollout-side HIP kernels of the PPO engine.
 *
 *   satrl_gae               <- ppo_continuous.py:198-210 (deltas, reversed GAE loop,
 *                              v_target = adv + vs), one lane per env, reverse scan
 *                              over the horizon of a time-major [T][N] buffer
 *   satrl_gaussian_sample   <- ppo_continuous.py:176-189 choose_action (Gaussian):
 *                              Normal(mean, exp(log_std)).sample() -> clamp(+-max)
 *                              -> per-dim log_prob; counter-based Philox4x32-10
 *                              keyed by (seed, agent, global env id, step), so a
 *                              rollout is identical for any env sharding
 *   satrl_moments           <- adv.mean() / adv.std() of ppo_continuous.py:210
 *                              (f64 sum and sum of squares, for a global all-reduce)
 *   satrl_obs_normalize     <- normalization.py:38-47 Normalization.__call__ with
 *                              frozen statistics, plus per-slot f64 moment sums
 *   satrl_return_scan       <- normalization.py:50-63 RewardScaling's running return
 *                              and its per-slot f64 moment sums
 *   satrl_episode_record    <- CPPO_main.py:233-282 test_network's bookkeeping
 *                              (epsiode_reward += r until done), per env: the
 *                              first episode's return, length, outcome, closest
 *                              and final distance and commanded delta-v
 *
 * All pointers are device buffers, calls are async on `stream` (hipStream_t,
 * NULL = default) and graph-capturable.  Return 0 or a negative error code.
 */
#ifndef SATRL_ROLLOUT_H
#define SATRL_ROLLOUT_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* r f32 [T][N], done u8 [T][N] (dw == done, CPPO_main.py:136-139 with the
 * env's own timeout), v f32 [T+1][N] = critic(obs[0..T]);  outputs adv and
 * v_target f32 [T][N].  f32 arithmetic in the reference's order, no FMA.   */
int satrl_gae(int64_t T, int64_t N, const float* r, const uint8_t* done, const float* v, float gamma, float lamda,
              float* adv_out, float* vtarget_out, void* stream);

/* mean f32 [N][3], log_std f32 [3]; act/logp f32 [N][3].  The Philox
 * counter's step is `step` plus, if step_base (a device u64) is non-NULL,
 * *step_base -- so a captured hipGraph replays with fresh noise once the
 * caller advances *step_base.                                              */
int satrl_gaussian_sample(int64_t N, const float* mean, const float* log_std, float max_action, uint64_t seed,
                          uint32_t agent, int64_t env_offset, uint64_t step, const uint64_t* step_base,
                          float* act_out, float* logp_out, void* stream);

/* out f64[2] += (sum x, sum x^2) over x f32 [n]  (out must be zeroed first) */
int satrl_moments(int64_t n, const float* x, double* out, void* stream);
/* The same sums, added in a fixed order: equal bits from call to call
 * (satrl_moments adds its blocks' sums with atomics, in the order the blocks
 * happen to finish, once n exceeds one block of 256).  scratch: a device
 * buffer of at least satrl_moments_scratch(n) doubles, overwritten; a smaller
 * scratch_elems returns -1 before any launch.  Two launches.                 */
int64_t satrl_moments_scratch(int64_t n);
int satrl_moments_ordered(int64_t n, const float* x, double* out, double* scratch, int64_t scratch_elems,
                          void* stream);

/* Running observation normalisation (normalization.py:38-47, frozen statistics).
 * raw, out f32 [N][18], two different buffers; stats f32 [2][18] (mean row,
 * inv_std row) and pivot f32 [18] are device buffers read on every launch, so
 * a captured hipGraph replays with whatever the caller last wrote there.
 * out = clamp((raw - mean) * inv_std, +-clip): one f32 subtract, one f32
 * multiply, no FMA; clip <= 0 = no clamp.  If acc is non-NULL (then pivot
 * must be too) it is f64 [ceil(N/32)][2][18]: for slot k (rows 32k .. 32k+31)
 * and every feature acc[k][0] += sum d, acc[k][1] += sum d*d with
 * d = (double)raw - (double)pivot, rows past N contributing nothing.  The
 * order of a slot's terms depends on the row's index in the slot only and
 * there are no atomics (a plain read-modify-write by the slot's owner; calls
 * are ordered by the stream), so acc is bitwise reproducible and a shard
 * starting at a multiple of 32 envs writes the unsharded run's slots.       */
int satrl_obs_normalize(int64_t N, const float* raw, const float* stats, float clip, float* out, const float* pivot,
                        double* acc, void* stream);

/* Discounted-return scan of RewardScaling (normalization.py:50-63): r f32
 * [T][N] and done u8 [T][N] time-major as satrl_gae reads them, one lane per
 * env, forward over t: R = gamma * R + (double)r[t][i] in f64 (no FMA), the
 * slot's sum of R and of R*R added to acc f64 [ceil(N/32)][2] (fixed in-slot
 * order, no atomics), then R = 0 where done[t][i].  carry f64 [N] is R on
 * entry (t = 0) and is written after t = T-1.                               */
int satrl_return_scan(int64_t T, int64_t N, const float* r, const uint8_t* done, double gamma, double* carry,
                      double* acc, void* stream);

/* Episode records of a policy evaluation: every env's FIRST episode after the
 * reset call, one lane per env, SoA planes.
 *   rec_f64 f64 [5][N]: ret (sum of rewards), final_dis, min_dis, dv_p, dv_e
 *                       (sums of (|a0| + |a1|) + |a2| of pa / ea, in f64)
 *   rec_i32 i32 [2][N]: length, outcome (0 running, 1 captured, 2 timed out)
 *   alive   i32 [1]:    the envs whose outcome is still 0
 * reset: ret = dv_p = dv_e = 0, min_dis = +inf, final_dis = NaN, length =
 * outcome = 0, *alive = N.  record (after a satenv_step without autoreset:
 * reward f64 [N] and done u8 [N] are its outputs, obs64 f64 [N][18] its
 * observation, pa / ea f32 [N][3] the actions it was given) touches only envs
 * with outcome 0: adds the reward and the two action sums in f64 in call
 * order, counts the step, takes dis = sqrt((o0*o0 + o1*o1) + o2*o2) of
 * obs64[i][0:3] into min_dis, and where done[i] stores final_dis = dis and
 * outcome = (reward == capture_reward) ? 1 : 2 -- the env writes its terminal
 * rewards as exact literals -- and takes the env off *alive (one vector atomic
 * per wave).  N <= 0 or a NULL pointer: -1 before any device call.         */
int satrl_episode_record_reset(int64_t N, double* rec_f64, int32_t* rec_i32, int32_t* alive, void* stream);
int satrl_episode_record(int64_t N, const double* reward, const uint8_t* done, const double* obs64, const float* pa,
                         const float* ea, double capture_reward, double* rec_f64, int32_t* rec_i32, int32_t* alive,
                         void* stream);

/* League tally: a rollout's finished episodes and captures per 32-env block,
 * from the rollout table itself.  rew f32 [T][N], done u8 [T][N]; for block
 * b (envs 32 b .. 32 b + 31, the ragged last block its valid envs only):
 *   tally[b][0] += steps (t, env) with done != 0
 *   tally[b][1] += those of them with rew == capture_reward
 * tally i64 [ceil(N/32)][2] on the device, added to.  capture_reward is the
 * f32 literal the env writes at a capture (it differs from the timeout's).
 * Integer sums: exact, independent of order and sharding; a block belongs to
 * one half-wave, so there are no atomics.  -1 before any device call: T or N
 * not positive, T above INT32_MAX (a lane counts in 32 bits), a NULL rew,
 * done or tally.                                                            */
int satrl_league_tally(int64_t T, int64_t N, const float* rew, const uint8_t* done, float capture_reward,
                       int64_t* tally, void* stream);

/* "<entry point>: <reason>" of this thread's last refused satrl_* call (the
 * slot satrl_ppo_last_error of satrl_ppo.h returns too).                  */
const char* satrl_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
