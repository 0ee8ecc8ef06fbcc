/*
 * satrl_ppo.h -- C ABI of the fused PPO minibatch-step kernels (gfx950).
 *
 * Replaces the per-minibatch body of PPO_continuous.update
 * (qiaobeibei/PPO-RL-Satellite ppo_continuous.py:213-239): actor
 * clipped-surrogate + entropy loss and critic MSE loss, their backward
 * passes, clip_grad_norm_(0.5) per net and Adam(eps) per net.  Actor and
 * critic (same hidden width H, tanh) are stepped together on the same
 * minibatch rows.  Per minibatch: satrl_ppo_rowpass (everything that is
 * row-parallel, incl. the two H x H products on f32 MFMA), satrl_ppo_dw2
 * (the dW2 weight gradient, split-K over rows), satrl_ppo_reduce and
 * satrl_ppo_adam.
 *
 * Flat parameter / gradient / Adam-moment layout (f32, see satrl_ppo_layout):
 *   W2   [2][H][H]     fc2.weight (actor, critic)
 *   W1   [2][H][20]    [fc1.weight(18) | fc1.bias | 0]  (actor, critic)
 *   b2   [2][H]        fc2.bias
 *   W3a  [3][H]        actor mean_layer.weight
 *   b3a  [4]           actor mean_layer.bias (3 used)
 *   ls   [4]           actor log_std (3 used)
 *   W3c  [H]           critic fc3.weight
 *   b3c  [4]           critic fc3.bias (1 used)
 * Gradients are produced as split-K partial slabs (dW2 from satrl_ppo_dw2
 * split S ways, [dW1|db1] and the "tail" b2..b3c (6H+12 floats) from
 * satrl_ppo_rowpass) and summed by satrl_ppo_reduce in a fixed order, so a
 * step is bitwise deterministic.  Packed transition rows (src) are [B][32] f32:
 * s(18) a(3) logp(3) adv(1) v_target(1) pad(6).
 */
#ifndef SATRL_PPO_H
#define SATRL_PPO_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { SATRL_PPO_OFF_W2 = 0, SATRL_PPO_OFF_W1, SATRL_PPO_OFF_B2, SATRL_PPO_OFF_W3A, SATRL_PPO_OFF_B3A,
       SATRL_PPO_OFF_LS, SATRL_PPO_OFF_W3C, SATRL_PPO_OFF_B3C, SATRL_PPO_TOTAL, SATRL_PPO_NOFF };

/* host helper: element offsets of the flat layout for hidden width H (64, 128 or 256) */
int satrl_ppo_layout(int H, int64_t* offsets /* [SATRL_PPO_NOFF] */);
/* number of partial slabs (row blocks: 32 rows, or 16 at H = 256 for mb <= 1024) the rowpass of a
 * minibatch of mb rows -- or of any shorter one -- writes, and of norm blocks */
int satrl_ppo_sizes(int H, int mb, int64_t* n_head_wg, int64_t* n_norm_blocks);

/* The plan of the product's minibatch step for (H, mb, net): which kernels
 * run and what every buffer must hold.  Host arithmetic only, no device call;
 * the one statement of every rule that picks a kernel or sizes a buffer (the
 * launches below take their kernel from it, satrl_ppo_sizes / _row_blocks /
 * _kx_elems / _dw2_kx_splits are reads of it).  A host sizes its buffers from
 * the plan of its longest minibatch and steps each minibatch, a ragged tail
 * too, with the `splits` of that minibatch's own plan.                     */
enum { SATRL_PPO_STEP_ROWS = 0,   /* rowpass -> dw2 -> reduce -> adam                       (H 128) */
       SATRL_PPO_STEP_FUSED,      /* rowpass_dw2 -> reduce -> adam                          (H 64)  */
       SATRL_PPO_STEP_KX };       /* rowpass_kx -> dw2_kx_w1 -> reduce(mode | 4) -> adam    (H 256) */
enum { SATRL_PPO_RP_WG32 = 0,     /* 32-row workgroups, workgroup barriers                          */
       SATRL_PPO_RP_WG16,         /* 16-row 16-wave workgroups                                      */
       SATRL_PPO_RP_CS,           /* column split when its grid is resident, else WG16 (same bits)  */
       SATRL_PPO_RP_WG32_HANDOFF };  /* 32-row workgroups, per-chunk LDS hand-offs                  */
typedef struct satrl_ppo_plan {
  int step, rowpass;              /* the enums above, for the product step of (H, mb, net)          */
  int rows_per_block, row_blocks; /* this minibatch                                                 */
  int splits;                     /* S of this minibatch's dW2 / reduce                             */
  int error_word;                 /* 1: the rowpass may set the word satrl_ppo_rowpass_error reads  */
  /* capacities that hold this minibatch AND every shorter one (a ragged tail), both nets:          */
  int64_t slab_blocks, norm_blocks, max_splits;
  int64_t ptail_floats, pw1_floats, p2_floats, kx_elems /* 0 unless KX */, rows_floats /* H1 or dZ2 f32 */;
} satrl_ppo_plan;
/* rowpass: the kernel satrl_ppo_rowpass_kx (KX), satrl_ppo_rowpass_dw2 (FUSED)
 * or satrl_ppo_rowpass (ROWS) launches for (H, mb, net), under the current
 * satrl_ppo_rowpass_sync mode; whether a column-split grid is resident is
 * settled at the launch, not here.  splits: satrl_ppo_row_blocks (FUSED),
 * satrl_ppo_dw2_splits (ROWS, the both-nets count for every net) or
 * satrl_ppo_dw2_kx_splits(H, mb, net) (KX).  max_splits >= the splits of every
 * minibatch of at most mb rows for this net: slab_blocks (FUSED), else at
 * least the dW2 kernel's workgroup target over its output tiles.  ptail_floats
 * = slab_blocks * (6H + 12), pw1_floats = slab_blocks * 2 * H * 20, p2_floats
 * = 2 * max_splits * H * H, rows_floats = 2 * mb * H, kx_elems per plane
 * buffer.  -1: H not 64/128/256, mb <= 0, net not -1/0/1 or a NULL plan.    */
int satrl_ppo_step_plan(int H, int mb, int net, satrl_ppo_plan* plan);

/* `net` (rowpass, reduce, adam): -1 = actor and critic in one launch, 0 =
 * actor only, 1 = critic only.  The two nets share nothing in a minibatch
 * step but the rows, and a one-net call touches only that net's elements
 * of every buffer, so the actor and critic chains may run concurrently on
 * two streams (each with its own nsq buffer).                              */

/* dW2 = dZ2^T H1 per net (the fc2 weight gradient) split-K S ways into the
 * slabs p2 [2][S][H][H] (f32 MFMA, fixed summation order) from the f32 rows
 * satrl_ppo_rowpass writes, at every width.  S must be
 * satrl_ppo_dw2_splits(H, mb) (about one workgroup per CU, no empty split).
 * The product paths (satrl_ppo_step_plan's step): H = 128 runs this entry
 * (ROWS), H = 64 fuses the product into the rowpass (FUSED,
 * satrl_ppo_rowpass_dw2, which H = 128 can run too), H = 256 runs it from
 * k-packed planes (KX, satrl_ppo_rowpass_kx + satrl_ppo_dw2_kx_w1).       */
int satrl_ppo_dw2_splits(int H, int mb);
/* Capacities (every call that writes or reads the dW2 slabs or the k-packed
 * planes takes the caller's buffer size and refuses with -1, before any
 * launch, when the call would run past it): p2_floats = elements of p2,
 * at least (net == 0 ? 1 : 2) * S * H * H; kx_elems = elements of EACH of
 * H1x / dZ2x, at least satrl_ppo_kx_elems(H, mb) (half of it for net 0).  */
int satrl_ppo_dw2(int H, int mb, int net, int S, const float* H1, const float* dZ2, float* p2, int64_t p2_floats,
                  void* stream);

/* mode 1: sum the partial slabs into G (p2: dW2 split-K [2][S][H][H], p1:
 * satrl_ppo_rowpass [dW1|db1] slabs, pt: satrl_ppo_rowpass tail slabs); mode 2: per-block
 * sums of squares of G per net into nsq [n_norm_blocks][2] (f64) and
 * advance steps [net] (f64); mode 3: both.  (mode 1 | all-reduce(G) | mode 2
 * under data parallelism.)  Every sum has a fixed order.  Mode bit 4 (with
 * 1 or 3): the W2 region only, after satrl_ppo_dw2_kx_w1 summed the W1 and
 * tail regions (p1 / pt may then be NULL).                                 */
int satrl_ppo_reduce(int H, int mb, int net, int S, int mode, const float* p2, int64_t p2_floats, const float* p1,
                     const float* pt, float* G, double* nsq, double* steps, void* stream);

/* Data parallelism, after the all-reduce (SUM) of G over `world` ranks:
 * G /= world (IEEE division, = torch's div_ of the gradient average), then
 * satrl_ppo_reduce mode 2 on it.  One launch, so mode 1 | ncclAllReduce |
 * this | satrl_ppo_adam is a single-stream chain a hipGraph captures whole.
 * Replaces the per-minibatch gradient of PPO_continuous.update
 * (ppo_continuous.py:227-239) for a minibatch spread over the ranks.       */
int satrl_ppo_reduce_dp(int H, int mb, int net, int world, float* G, double* nsq, double* steps, void* stream);

/* clip_grad_norm_(max_norm) per net (use_clip) + torch Adam (lerp form) per
 * net: lr [2] f32 device; bct f64 [bct_len][2] = {1 - beta1**k, sqrt(1 -
 * beta2**k)} for step k computed on the host with python-float math (as
 * torch.optim.Adam does), 1.0 past the table.                             */
int satrl_ppo_adam(int H, int mb, int net, const double* nsq, const double* steps, const double* bct, int bct_len,
                   const float* lr, float beta1, float beta2, float eps, float max_norm, int use_clip, const float* G,
                   float* P, float* M, float* V, void* W2X /* nullable: also refresh the fc2 operand image */,
                   void* stream);

/* The fc2 operand image W2X the rowpass reads for its two H x H products
 * (and satrl_ppo_adam keeps current), satrl_ppo_w2x_floats(H) floats: the
 * f32 fc2.weight^T per net, [2][H][H], at every width (phase D's B operand;
 * at H = 256 the rowpass splits it into bf16 planes in registers -- a
 * pre-split planes image measured slower).
 * satrl_ppo_w2x_sync builds it from P (net -1: both) -- after a load or any
 * write to fc2.weight outside satrl_ppo_adam.  The rowpass relies on the
 * image being P's fc2.weight transposed: where it skips phase D
 * (satrl_ppo_rowpass_dskip) it bounds the image's elements by the
 * fc2.weight elements its forward pass loaded from P.                      */
int64_t satrl_ppo_w2x_floats(int H);
int satrl_ppo_w2x_sync(int H, int net, const float* P, void* W2X, void* stream);

/* The row-parallel part of one minibatch step in ONE launch (a workgroup
 * per net and 32-row block): gather + fc1 + tanh, fc2 (f32 MFMA; split-bf16
 * at H = 256), output layer, the net's loss and gradients, backprop through
 * fc2 (the fc2 operand image W2X, above) and tanh(fc1).  Rows are
 * src[idx[r]] (idx nullable: rows 0..mb-1 of src, contiguous).  Writes H1
 * and dZ2 [2][mb][H] (inputs of the dW2 GEMM), the tail partial slabs
 * [n_head_wg][6H+12] and the [dW1 | db1] partial slabs [n_head_wg][2][H][20]
 * (n_head_wg from satrl_ppo_sizes).                                      */
int satrl_ppo_rowpass(int H, int mb, int net, const float* src, const int64_t* idx, const float* P, const void* W2X,
                      float epsilon, float ent_coef, float max_action, float* H1, float* dZ2, float* ptail,
                      float* pw1, void* stream);

/* The same launch for the actor's probability ratios: ratio f32 [mb]
 * (row order of the minibatch) receives exp(logp(a|s) - logp_old) of every
 * row as the loss head computes it (ppo_continuous.py:220); the other
 * outputs are satrl_ppo_rowpass's.  The parity hook of the identity "the
 * first epoch's first minibatch recomputes the rollout's log-probs bit for
 * bit", i.e. every ratio == 1.0f exactly.  net must include the actor.    */
int satrl_ppo_rowpass_ratio(int H, int mb, int net, const float* src, const int64_t* idx, const float* P,
                            const void* W2X, float epsilon, float ent_coef, float max_action, float* H1, float* dZ2,
                            float* ptail, float* pw1, float* ratio, void* stream);

/* H = 64 / 128 (BASELINE configs[1]): the rowpass with the dW2 product fused
 * in.  Each workgroup multiplies its own 32 rows' dZ2^T H1 out of LDS and
 * writes that partial as split-K slab (its row block) of p2 [2][S][H][H],
 * S = satrl_ppo_row_blocks(H, mb); H1 / dZ2 are not written.  The slabs are
 * bitwise satrl_ppo_dw2's at that S (one 32-row chunk per split, the same
 * MFMA sequence), so satrl_ppo_reduce(..., S, ...) gives the same G; the
 * minibatch step is three launches (rowpass_dw2, reduce, adam).            */
int satrl_ppo_row_blocks(int H, int mb);
int satrl_ppo_rowpass_dw2(int H, int mb, int net, const float* src, const int64_t* idx, const float* P,
                          const void* W2X, float epsilon, float ent_coef, float max_action, float* p2,
                          int64_t p2_floats /* >= (net == 0 ? 1 : 2) * S * H * H */, float* ptail, float* pw1,
                          void* stream);

/* H = 256, every minibatch (32-row workgroups above 1024 rows, 16-row ones
 * up to it): the rowpass with H1 and dZ2 written as k-packed bf16 planes (each element split hi + mid +
 * lo exactly; element (r, n) of a net's plane at ((r/8)*H + n)*8 + r%8,
 * rows padded with zeros to whole 32-row chunks): u16 H1x / dZ2x
 * [2][3][ceil(mb/32)*32][H], satrl_ppo_kx_elems(H, mb) elements each.
 * satrl_ppo_dw2_kx multiplies them into the dW2 split-K slabs p2
 * [2][S][H][H] on the split-bf16 MFMA (the fc2 products' arithmetic: error
 * below an f32 MFMA chain's), S = satrl_ppo_dw2_kx_splits(H, mb, net); the
 * minibatch step is then rowpass_kx, dw2_kx, reduce(S), adam.              */
int64_t satrl_ppo_kx_elems(int H, int mb);
int satrl_ppo_rowpass_kx(int H, int mb, int net, const float* src, const int64_t* idx, const float* P, const void* W2X,
                         float epsilon, float ent_coef, float max_action, void* H1x, void* dZ2x, int64_t kx_elems,
                         float* ptail, float* pw1, void* stream);
int satrl_ppo_dw2_kx_splits(int H, int mb, int net);
int satrl_ppo_dw2_kx(int H, int mb, int net, int S, const void* H1x, const void* dZ2x, int64_t kx_elems, float* p2,
                     int64_t p2_floats, void* stream);
/* satrl_ppo_dw2_kx and satrl_ppo_reduce's W1 / tail regions in one launch
 * (their slabs p1 / pt are the rowpass's, ready before dW2 runs): G's W1 and
 * tail parts, and with mode 3 their squared-norm pairs in nsq; then
 * satrl_ppo_reduce(..., mode | 4, ...) sums the W2 region.  Bitwise the
 * dw2_kx + reduce(mode) pair.  mode 1 or 3.                                */
int satrl_ppo_dw2_kx_w1(int H, int mb, int net, int S, const void* H1x, const void* dZ2x, int64_t kx_elems, float* p2,
                        int64_t p2_floats, int mode, const float* p1, const float* pt, float* G, double* nsq,
                        void* stream);
/* Up to 1024 rows (configs[3]'s per-rank minibatch, the 16-row range),
 * both nets, when its grid is resident at once, satrl_ppo_rowpass_kx runs
 * the column-split kernel: each (16-row block, net) on four workgroups of
 * four waves, one per 64 hidden columns, which exchange the output-layer
 * partials and the dZ2
 * planes inside the launch (bitwise the 16-wave kernel's outputs).  Its
 * exchange state is the library's own, per device: launches of it must not
 * run concurrently on two streams of one device.  A wait that times out
 * (0.5 s; a grid not co-resident) leaves the kernel with its outputs invalid
 * and sets an error word: satrl_ppo_rowpass_error waits for the stream
 * (at most timeout_s seconds of host time: -2 when it has not drained by
 * then, e.g. behind a collective of a dead peer), reports the word in *err
 * (1; 0 = none), and on an error re-arms the exchange state (the update
 * that saw it must be discarded).                                          */
int satrl_ppo_rowpass_error(int* err, double timeout_s, void* stream);
/* Development switch (A/B timing, and the tests' bitwise oracle): how the
 * phases of the 32-row 16-wave k-packed rowpass kernel (satrl_ppo_rowpass_kx
 * above 1024 rows) wait for each other inside a workgroup.  0: workgroup
 * barriers; 1: per-chunk LDS hand-offs (the same kernel source, every output
 * bit the same; a hand-off wait that runs out -- never, unless the kernel
 * is wrong -- sets the error word satrl_ppo_rowpass_error reports and the
 * kernel still ends).  Process-wide, read at launch (a captured graph keeps
 * the form it was captured with).  Returns the previous mode; mode -1 only
 * queries; anything else -1.                                               */
int satrl_ppo_rowpass_sync(int mode);
/* A second development switch (A/B timing, and the tests' bitwise oracle),
 * outside the declared ABI: whether a
 * wave of that 32-row kernel, in either sync form, may skip phase D (dH1 =
 * dZ2 W2) and phase E's products and store +0.0 to its [dW1 | db1] slab
 * rows.  It does so only where every output byte is the full path's: its own
 * 32 x 16 tile of tanh(fc1) is exactly +-1 (fc1 saturated, as with raw-metre
 * observations: dZ1 = dH1 x 0), the block's states are finite, and the
 * exponents of the block's dZ2 and of the net's fc2.weight bound dH1 to
 * finite values.  0: phase D always runs; 1: the default.  Process-wide, read
 * at launch (a captured graph keeps the mode it was captured with).  Returns
 * the previous mode; mode -1 only queries; anything else -1 with a message
 * that names it.  The library exports it as
 *     int satrl_ppo_rowpass_dskip(int mode)
 * for the package's helper (satrl.ppo.rowpass_dskip) and the tests; it is not
 * declared here: a call with mode 0 succeeds and changes the process, which
 * no entry point of this ABI does when every argument is zero.             */
/* satrl_ppo_rowpass_kx on that 32-row kernel whatever the minibatch size (the
 * kernel tests' entry: one block, ragged blocks, either block placement), in
 * the form satrl_ppo_rowpass_sync selects: ceil(mb / 32) slabs of ptail / pw1
 * (never more than satrl_ppo_sizes gives), the planes as satrl_ppo_rowpass_kx,
 * and the actor's per-row ratio in ratio [mb] (nullable).                  */
int satrl_ppo_rowpass_kx32(int H, int mb, int net, const float* src, const int64_t* idx, const float* P,
                           const void* W2X, float epsilon, float ent_coef, float max_action, void* H1x, void* dZ2x,
                           int64_t kx_elems, float* ptail, float* pw1, float* ratio, void* stream);
/* Fault injection for tests: sets (row block, net) group `group`'s exchange
 * counter to `value` (synchronising the stream).  A value that breaks the
 * counter's invariant (a multiple of 8 at every launch's start, e.g. 5)
 * makes that group's next launch wait out its timeout, set the error word
 * and leave the kernel: the path satrl_ppo_rowpass_error reports.        */
int satrl_ppo_rowpass_fault_inject(int group, unsigned value, void* stream);

/* Rollout forward passes on the rowpass's own MLP code, so every row's result
 * is independent of N and of the sharding, and the rollout's log-probs equal
 * the update's first recomputation bit for bit.
 * satrl_policy_act <- CPPO_main.py:122-123 (both agents' choose_action,
 * ppo_continuous.py:176-189): for the actor (net 0) of each flat parameter
 * set P0 (pursuer, agent 0) and P1 (evader, agent 1; nullable = one agent),
 * mean = max_action*tanh(mean_layer), a = clamp(mean + exp(log_std)*z,
 * +-max_action), per-dim Normal log-prob; z from Philox4x32-10 keyed by
 * (seed, agent, env_offset + row, step + *step_base) exactly as
 * satrl_gaussian_sample.  obs f32 [N][18], act/logp f32 [N][3].           */
int satrl_policy_act(int H, int64_t N, const float* obs, const float* P0, const float* P1, float max_action,
                     uint64_t seed, int64_t env_offset, uint64_t step, const uint64_t* step_base, float* act0,
                     float* logp0, float* act1, float* logp1, void* stream);
/* satrl_policy_act with an opponent pool: agent pool_agent (0 | 1) acts, per
 * 32-row block, with a stored parameter set instead of its live one.  pool is
 * f32 [K][pool_stride], each row a flat parameter set in satrl_ppo_layout's
 * order; member i32 [ceil(N / 32)] (device) names block b's row:
 *   m = member[b];  P = 0 <= m < K ? pool + m * pool_stride : the live P0 / P1
 * Every m outside [0, K) (-1, K, INT_MIN, anything) means the live
 * parameters; no value of m makes the kernel read outside pool.  The other
 * agent, the Philox key and counter, env_offset, step and step_base are
 * exactly satrl_policy_act's, so a block's rows are bit for bit those of
 * satrl_policy_act called with that block's parameter set.  The granularity
 * is a block because a workgroup streams one net's weights for its 32 rows.
 * member and pool are read at every launch: a captured graph follows in-place
 * changes of either with no recapture.
 * -1 before any device call (satrl_ppo_last_error says which): every refusal
 * of satrl_policy_act; a NULL P1, act1 or logp1 (both agents are required);
 * pool_agent not 0 or 1; a NULL pool or member; K <= 0; pool_stride below
 * SATRL_PPO_TOTAL of satrl_ppo_layout(H) or not a multiple of 4; pool not
 * 16-byte aligned.
 * Span probe: the pooled kernel has no probed instantiation.  While a span
 * probe is set (satrl_span_probe) a pooled launch runs the product kernel and
 * adds nothing to the launch log.                                          */
int satrl_policy_act_pool(int H, int64_t N, const float* obs, const float* P0, const float* P1, float max_action,
                          uint64_t seed, int64_t env_offset, uint64_t step, const uint64_t* step_base, float* act0,
                          float* logp0, float* act1, float* logp1, int pool_agent /* 0 | 1 */,
                          const float* pool /* [K][pool_stride] */, int64_t pool_stride, int K,
                          const int32_t* member /* [ceil(N/32)], device, read at every launch */, void* stream);
/* Which stored opponent each 32-env block plays this iteration.  Host only, no
 * device call.  For global block g = first_block + i, i < n_blocks:
 *   w = philox4x32_10(counter {lo32(g), hi32(g), lo32(iteration),
 *       hi32(iteration)}, key of (seed, stream 3))   (streams 0 / 1: the action
 *       noise, 2: the reset draw)
 *   u = (w[0] + 0.5) * 2^-32
 *   member_out[i] = filled == 0 || u < latest_prob ? -1 : (w[1] * filled) >> 32
 * so an assignment depends on (seed, iteration, g, filled, latest_prob) alone
 * and not on how the envs are sharded.  -1: a NULL output, n_blocks <= 0,
 * first_block < 0, filled < 0, latest_prob outside [0, 1] or NaN.          */
int satrl_opponent_assign(uint64_t seed, uint64_t iteration, int64_t first_block, int64_t n_blocks, int filled,
                          double latest_prob, int32_t* member_out /* host */);
/* satrl_policy_eval <-PPO_continuous.evaluate (ppo_continuous.py:168-174) on
 * satrl_policy_act's forward path, block shape and agent interleave; actions
 * only, no log-probs.  Agent a (0: P0, 1: P1) with bit 1 << a of det_mask
 * set acts with the mean, a = max_action*tanh(mean_layer); an agent whose bit
 * is clear samples, and its action is bit for bit the one satrl_policy_act
 * writes for the same (seed, agent, env_offset + row, step + *step_base).
 * -1 before any device call: H not 64/128/256, N <= 0, a NULL obs, P0 or
 * act0, det_mask outside 0..3, bit 1 set without P1, P1 without act1.     */
int satrl_policy_eval(int H, int64_t N, const float* obs, const float* P0, const float* P1, float max_action,
                      int det_mask, uint64_t seed, int64_t env_offset, uint64_t step, const uint64_t* step_base,
                      float* act0, float* act1, void* stream);
/* Scripted opponents: a linear guidance law in place of a network.  Per env
 * row, over its 18 RAW observation features s (metres, m/s -- never the
 * normalised row a learner may see) and action dimension d:
 *   acc = b[d];  for j = 0..17 ascending: acc = acc + G[d][j] * (double)s[j]
 *   act[d] = (float) (acc < -m ? -m : acc > m ? m : acc),  m = max_action
 * every product rounded to f64 and then the sum (no fused multiply-add), the
 * final conversion round-to-nearest-even; a NaN acc passes the clamp.  The
 * fixed-horizon intercept and flee laws, coasting and constant thrust are
 * all of this form (satrl/scripted.py builds G from satenv_stm).           */
typedef struct satrl_scripted_law {   /* 58 doubles, 464 B */
  double G[3][18];                    /* row d: weights over the 18 raw observation features */
  double b[3];
  double max_action;                  /* > 0 */
} satrl_scripted_law;
/* act f32 [N][3] = the law over obs f32 [N][18]; `law` is a DEVICE block, read
 * at the launch (a captured graph follows in-place changes of it with no
 * recapture).  -1 before any device call: N <= 0, a NULL obs, law or act.  */
int satrl_scripted_act(int64_t N, const float* obs, const satrl_scripted_law* law, float* act, void* stream);
/* The same source through the host compiler on HOST pointers: the same bits,
 * no device call (the arithmetic's test hook).  -1 as above.               */
int satrl_scripted_act_host(int64_t N, const float* obs, const satrl_scripted_law* law, float* act);
/* satrl_policy_act for ONE learning agent against a scripted one, in one
 * launch.  Agent `agent` (0 pursuer | 1 evader) acts with the flat parameter
 * set P on obs: its rows of act / logp are bit for bit those satrl_policy_act
 * writes for that agent (its Philox key stream, the same counter, env_offset,
 * step, step_base, block shape and forward code).  The other agent's rows,
 * act_scripted f32 [N][3], are bit for bit satrl_scripted_act(obs_law, law):
 * a tail of extra workgroups that branch uniformly round the MLP, never touch
 * P and write no log-prob.  obs_law (the raw observation) may equal obs.
 * `law` is a device block, read at every launch.
 * -1 before any device call (satrl_ppo_last_error says which): every refusal
 * of satrl_policy_act (H not 64/128/256, N <= 0, a NULL obs, P, act or logp);
 * a NULL obs_law, law or act_scripted; agent not 0 or 1.
 * Span probe: as the pooled kernel, no probed instantiation; nothing is
 * logged for these launches.                                               */
int satrl_policy_act_scripted(int H, int64_t N, const float* obs, const float* obs_law, const float* P,
                              int agent /* the learner: 0 | 1 */, float max_action, uint64_t seed, int64_t env_offset,
                              uint64_t step, const uint64_t* step_base, float* act, float* logp,
                              const satrl_scripted_law* law /* device */, float* act_scripted, void* stream);
/* The same for satrl_policy_eval, actions only: det = 1, agent `agent` acts
 * with its mean; det = 0, it samples, bit for bit as in satrl_policy_eval.
 * -1 as above (no logp), and for det not 0 or 1.                            */
int satrl_policy_eval_scripted(int H, int64_t N, const float* obs, const float* obs_law, const float* P,
                               int agent /* 0 | 1 */, float max_action, int det /* 0 | 1 */, uint64_t seed,
                               int64_t env_offset, uint64_t step, const uint64_t* step_base, float* act,
                               const satrl_scripted_law* law /* device */, float* act_scripted, void* stream);
/* League play: satrl_policy_act_pool with a table of J laws behind the K
 * stored sets.  Per 32-row block b of agent pool_agent, m = member[b]:
 *   0 <= m < K       the stored set pool + m * pool_stride, as the pooled call
 *   K <= m < K + J   law j = m - K: the workgroup branches uniformly round the
 *                    whole MLP (no parameter, no LDS, no barrier); rows r of
 *                    the block get act = the law laws[j] over obs_law's row
 *                    (bit for bit satrl_scripted_act) and logp = +0.0f
 *   anything else    (-1, K + J, INT_MIN, ...) the live P0 / P1
 * No value of m makes the kernel read outside pool or laws.  A stored or live
 * block's rows and all of the other agent's rows are bit for bit those of
 * satrl_policy_act with that block's parameter set; the Philox keys, the
 * counter, env_offset, step and step_base are satrl_policy_act_pool's.
 * obs_law f32 [N][18] is the raw observation and may equal obs; laws is a
 * DEVICE array satrl_scripted_law[J].  member, pool and laws are read at every
 * launch: a captured graph follows in-place changes of all three with no
 * recapture.
 * -1 before any device call (satrl_ppo_last_error says which): every refusal
 * of satrl_policy_act_pool; a NULL obs_law or laws; J outside
 * 1 .. SATRL_LEAGUE_MAX_LAWS; laws not 8-byte aligned.
 * Span probe: as the pooled kernel, no probed instantiation; nothing is
 * logged for these launches.                                               */
#define SATRL_LEAGUE_MAX_LAWS 8
int satrl_policy_act_league(int H, int64_t N, const float* obs, const float* P0, const float* P1, float max_action,
                            uint64_t seed, int64_t env_offset, uint64_t step, const uint64_t* step_base, float* act0,
                            float* logp0, float* act1, float* logp1, int pool_agent /* 0 | 1 */,
                            const float* pool /* [K][pool_stride] */, int64_t pool_stride, int K,
                            const int32_t* member /* [ceil(N/32)], device */, const float* obs_law,
                            const satrl_scripted_law* laws /* [J], device */, int J, void* stream);
/* Which league member each 32-env block plays this iteration: the rule of
 * satrl_opponent_assign with laws and weighted stored opponents.  Host only.
 * For global block g = first_block + i, with w and u as satrl_opponent_assign
 * forms them (the same Philox word), in this order:
 *   1. (filled == 0 && n_laws == 0) || u < latest_prob:          m = -1
 *   2. n_laws > 0 && (filled == 0 || u < latest_prob + law_prob): m = K + ((w[2] * n_laws) >> 32)
 *   3. weights == NULL:                                          m = (w[1] * filled) >> 32
 *   4. else, S = weights[0] + .. + weights[filled - 1] in f64, ascending k,
 *      v = (w[1] + 0.5) * 2^-32 * S: m = the first k whose running sum c_k has
 *      v < c_k, and the last k with weights[k] > 0 when none has.
 * With n_laws == 0 and weights == NULL the output is satrl_opponent_assign's.
 * It depends on (seed, iteration, g, K, filled, n_laws, the probabilities,
 * weights) alone, never on the sharding.  weights is read when filled > 0.
 * -1: a NULL member_out; n_blocks <= 0; first_block < 0; K < 0; filled outside
 * 0 .. K; n_laws outside 0 .. SATRL_LEAGUE_MAX_LAWS; latest_prob or law_prob
 * outside [0, 1] or NaN; latest_prob + law_prob > 1; a weight that is
 * negative or not finite; a weight sum that is not positive.               */
int satrl_league_assign(uint64_t seed, uint64_t iteration, int64_t first_block, int64_t n_blocks, int K, int filled,
                        int n_laws, double latest_prob, double law_prob,
                        const double* weights /* NULL | host [filled] */, int32_t* member_out /* host */);
/* critic value v f32 [N] of the flat parameters P (net 1) <- self.critic(s),
 * ppo_continuous.py:200-201                                               */
int satrl_policy_value(int H, int64_t N, const float* obs, const float* P, float* v_out, void* stream);

/* Update diagnostics: what an update did to the policy and the critic, from
 * the forward pass of both nets over n rows src[idx[r]] of the packed table
 * (idx nullable: rows 0..n-1, as satrl_ppo_rowpass).  Forward only, on the
 * rowpass's own gather and MLP code in the policy kernel's shape (a workgroup
 * per 32-row block and net), so every ratio is the bits the loss head would
 * form and every v the bits of satrl_policy_value; nothing of the update is
 * read but P and nothing written.  The pad columns of src are never read.
 * Per row, in f32 exactly as the loss head: d = logp(a|s) - logp_old, ratio =
 * expf(d), s1 = ratio*adv, s2 = clamp(ratio, 1 -+ epsilon)*adv, v = critic(s);
 * then in f64 from those f32 values the slots of sums f64 [SATRL_DIAG_N]:
 *   ROWS      n
 *   SURR      sum min(s1, s2)          (policy loss = -SURR / n)
 *   KL        sum (ratio - 1) - d      (the k3 estimator of KL(old || new))
 *   LOGRATIO  sum d
 *   CLIPPED   rows with ratio < 1 - epsilon or ratio > 1 + epsilon
 *   RATIO_MAX max ratio
 *   VERR2     sum (v - vt)^2           (value loss = VERR2 / n)
 *   VERR      sum (vt - v)
 *   VT, VT2   sum vt, sum vt^2
 * No atomics: each block adds its 32 rows in row order into a line of
 * scratch (f64, at least satrl_ppo_diagnostics_scratch(n) elements), and one
 * or (above 4096 blocks) two small launches add the lines in a fixed order,
 * so sums is bitwise reproducible for equal (n, src, idx, P).
 * rows_out (nullable) f32 [n][4] = ratio, d, v, 0 in the call's row order:
 * the parity hook, as satrl_ppo_rowpass_ratio's ratio.
 * Asynchronous on `stream`, no host synchronisation.  -1 before any device
 * call (and satrl_ppo_last_error set): H not 64/128/256, n <= 0 or above
 * 2^31 - 65, a NULL src, P, sums or scratch, scratch_len too small.        */
enum { SATRL_DIAG_ROWS = 0, SATRL_DIAG_SURR, SATRL_DIAG_KL, SATRL_DIAG_LOGRATIO, SATRL_DIAG_CLIPPED,
       SATRL_DIAG_RATIO_MAX, SATRL_DIAG_VERR2, SATRL_DIAG_VERR, SATRL_DIAG_VT, SATRL_DIAG_VT2, SATRL_DIAG_N };
int64_t satrl_ppo_diagnostics_scratch(int64_t n);
int satrl_ppo_diagnostics(int H, int64_t n, const float* src, const int64_t* idx, const float* P, float epsilon,
                          float max_action, double* sums, double* scratch, int64_t scratch_len, float* rows_out,
                          void* stream);

/* Minibatch staging for a graph-replayed group of minibatches
 * (BatchSampler(SubsetRandomSampler) order, ppo_continuous.py:217): rows
 * [0, rows) of stage f32 [rows][32] = src[perm[group[0] * rows + r]] (packed
 * transition rows, 32 f32 each), with group a device i64 counter, so the
 * replayed graph walks the epoch's permutation without a host copy.
 * satrl_ppo_group_advance: group[0] += 1 (the last node of such a graph).  */
int satrl_ppo_stage(int64_t rows, const float* src, const int64_t* perm, const int64_t* group, float* stage,
                    void* stream);
int satrl_ppo_group_advance(int64_t* group, void* stream);

/* y[i] = tanh(x[i]) f32 [n], with the activation every MLP kernel above uses
 * for torch.tanh in Actor_Gaussian / Critic.forward (ppo_continuous.py:61-134):
 * the hook of its exhaustive accuracy test.                               */
int satrl_ppo_tanh(int64_t n, const float* x, float* y, void* stream);
/* Test hook of the wave-uniform arm selection (tanh_f32_n, ppo_kernels.hip):
 * thread i takes x[8i .. 8i+7], the eight values of an MLP call site, so a
 * wave is 512 consecutive values; n a multiple of 8.  form 0: the
 * straight-line two-arm tanh on each value (satrl_ppo_tanh's function),
 * form 1: the per-wave arm selection on the eight.  The two must agree bit
 * for bit.                                                                 */
int satrl_tanh_forms(const float* x, float* y, int64_t n, int form, void* stream);

/* Live launch spans (measurement only; bench.py): while a probe buffer is
 * set, every launch of the rowpass, dW2 (k-packed), reduce, Adam, policy /
 * value and env-step (satenv.h) kernels -- eager or captured into a graph --
 * runs the kernel's SPAN instantiation, which differs from the product one
 * only in that lane 0 of every wave stores the wave's (start, exit)
 * s_memrealtime pair (100 MHz) into a region of the buffer of its own: 2
 * u64 per wave, regions taken in launch order.  A graph captured meanwhile
 * keeps its regions: each replay rewrites them.  satrl_span_probe(buf,
 * bytes, stream) zeroes buf on `stream` and starts the log; (NULL, 0) stops
 * probing (launches run the product instantiations again).  Launch i of the
 * log: its kernel kind (0 rowpass, 1 dW2, 2 reduce, 3 Adam, 4 policy_act, 5
 * policy_value, 6 env step), the u64 offset of its records and its wave
 * count; its span = max(exit) - min(start) over its waves.                */
int satrl_span_probe(void* buf, int64_t bytes, void* stream);
int64_t satrl_span_probe_launches(void);
int satrl_span_probe_launch(int64_t i, int* kind, int64_t* word_offset, int64_t* waves);

/* Every negative return of a satrl_* entry point (this header, satrl_peer.h,
 * satrl_rollout.h) leaves "<entry point>: <reason>" in one per-thread slot;
 * satrl_ppo_last_error and satrl_last_error both return it.               */
const char* satrl_ppo_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
