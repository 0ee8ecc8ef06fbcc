// ppo_kernels.hip -- fused PPO minibatch-step kernels for gfx950 (include/satrl_ppo.h).
//
// Per minibatch (actor + critic together, same rows), four launches:
//   rowpass  gather, fc1, fc2 (f32 MFMA), output layers, losses, backprop to
//            dZ2 and through fc2 (f32 MFMA) and fc1's tanh; writes H1, dZ2
//            and partial slabs of every small gradient
//   dW2      dZ2^T @ H1 split-K S ways: fused into the rowpass (H <= 128, rowpass_dw2), from the
//            rowpass's k-packed bf16 planes (H = 256, dw2_kx_kernel), or dw2_kernel on f32 rows
//   reduce   partial slabs -> G (fixed order), per-block squared norms per net
//   adam     clip coefficient per net + Adam (torch single-tensor formula),
//            also refreshes fc2.weight^T used by the next rowpass
// Every reduction has a fixed order, so a step is bitwise reproducible.
#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <cmath>
#include <cstring>
#include <cstdlib>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <utility>
#include <vector>

#include "philox_device.h"
#include "satrl_error.h"
#include "span_probe.h"
#include "satrl_ppo.h"
#include "satrl_peer.h"
#include "scripted_device.h"

namespace {

#ifdef SATRL_PHASE_PROBE
// development-only phase stamps (tools/_probe/phase_probe.py), never in the
// shipped build: [workgroup][stamp][wave][s_memrealtime, s_memtime]
__device__ unsigned long long g_probe[512][16][16][2];
#define PHASE_PROBE(k)                                                        \
  do {                                                                        \
    if ((threadIdx.x & 63) == 0 && blockIdx.x < 512) {                        \
      g_probe[blockIdx.x][k][threadIdx.x >> 6][0] = wall_clock64();           \
      g_probe[blockIdx.x][k][threadIdx.x >> 6][1] = clock64();                \
    }                                                                         \
  } while (0)
#else
#define PHASE_PROBE(k) do {} while (0)
#endif

constexpr int kRows = 32;     // minibatch rows per rowpass workgroup (and per partial slab)
constexpr int kNW256 = 16;    // waves per rowpass workgroup at H = 256
// short minibatches at H = 256 (configs[3]: 512 rows per rank; ragged tails)
// run 16-row workgroups of the same 16 waves, one 16-row tile each: twice the
// workgroups on the chip, and every row's arithmetic -- the forward's MFMA
// order and output-layer sums included -- is the 32-row kernel's
constexpr int kRowsShort = 16;

constexpr float kLogSqrt2Pi = 0.9189385332046727f;   // math.log(math.sqrt(2*math.pi))

struct Layout {
  int64_t W2, W1, b2, W3a, b3a, ls, W3c, b3c, total, tail;
};

__host__ __device__ inline Layout layout(int H) {
  Layout L;
  L.W2 = 0;
  L.W1 = L.W2 + 2LL * H * H;
  L.b2 = L.W1 + 2LL * H * 20;
  L.W3a = L.b2 + 2LL * H;
  L.b3a = L.b2 + 5LL * H;
  L.ls = L.b3a + 4;
  L.W3c = L.ls + 4;
  L.b3c = L.W3c + H;
  L.total = L.b3c + 4;
  L.tail = L.total - L.b2;   // 6H + 12
  return L;
}

// 0 = actor, 1 = critic (pads belong to the net of their segment)
__device__ __forceinline__ int net_of(const Layout& L, int64_t e, int H) {
  if (e < L.W1) return e >= (int64_t)H * H;
  if (e < L.b2) return (e - L.W1) >= (int64_t)H * 20;
  if (e < L.W3a) return (e - L.b2) >= H;
  return e >= L.W3c;
}

// ---------------------------------------------------------------------------
// rowpass: the whole row-parallel part of a minibatch step in one launch.
// The actor and critic losses are independent given (adv, v_target), so a
// workgroup owns ONE net (blockIdx & 1; with round-robin dispatch the actor
// lands on the even XCDs, the critic on the odd ones) and 32 minibatch rows
// (blockIdx >> 1).  Its NW waves split the hidden columns: wave w owns
// CT = H/16/NW tiles of 16 columns for both 16-row tiles.  Every CU thus
// streams one net's fc2 weights per phase (256 KB at H=256) for 32 rows:
// the two MFMA phases are L2->CU ingest bound.
//   A  gather rows -> S (LDS); Z1 = [S|1] W1aug^T       f32 MFMA 16x16x4
//   B  Z2 = tanh(Z1) W2^T                               f32 MFMA, W2 from L2
//   C  tanh(fc2), output layer(s), the net's loss, dZ2 -> LDS/HBM, tail partials
//   D  dH1 = dZ2 W2 (rows of W2T = fc2.weight^T)        f32 MFMA
//   E  dZ1 = dH1 (1 - H1^2); [dW1|db1] = dZ1^T [S|1]    f32 MFMA, dZ1's
//      accumulator layout is already the A operand
// Accumulator layout of a 16x16x4 tile: acc[rt][ct][j] = D[row 16rt + 4lg + j]
// [col n0 + 16ct + li].  Inside a 32-wide k chunk lane group g takes
// k = 32c + 8g + kk (kk < 8): every B fetch is a 32-B run of a 128-B line and
// A comes as 2 ds_read_b128 per row tile from rows padded by 16 B.
// Partial slabs are per 32-row block: the actor and critic workgroups of a
// block write disjoint parts of the same slab.
// ---------------------------------------------------------------------------
using f4 = __attribute__((ext_vector_type(4))) float;

__device__ __forceinline__ f4 mfma4(float a, float b, f4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// sum over the 16 lanes of a DPP row (lanes 16k .. 16k+15), result in every
// lane of the row: xor-1 and xor-2 quad permutes, then half-row and row
// mirrors -- VALU DPP, no LDS traffic (ds_bpermute chains were the slowest
// part of the output-layer dot products).  Fixed order, so deterministic.
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
__device__ __forceinline__ float row16_sum(float v) {
  v += dpp_f<0xB1>(v);    // quad_perm [1,0,3,2]
  v += dpp_f<0x4E>(v);    // quad_perm [2,3,0,1]
  v += dpp_f<0x141>(v);   // row_half_mirror
  v += dpp_f<0x140>(v);   // row_mirror
  return v;
}
// v + v[lane ^ 16] and v + v[lane ^ 32] by the gfx950 permlane swaps (VALU,
// no ds_bpermute round trip); fp addition commutes, so every lane's bits are
// those of v + __shfl_xor(v, 16 / 32)
__device__ __forceinline__ float xor16_sum(float v) {
  const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ __forceinline__ float xor32_sum(float v) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
// row16_sum of NV values stage by stage: NV independent DPP adds between
// dependent ones, so no DPP read-after-write s_nop is needed (value-major
// order left ~90 of them in phase C); every value's ops and order are the
// same as row16_sum's, so the sums are bitwise identical
template <int NV>
__device__ __forceinline__ void row16_sum_n(float (&v)[NV]) {
#pragma unroll
  for (int q = 0; q < NV; ++q) v[q] += dpp_f<0xB1>(v[q]);
#pragma unroll
  for (int q = 0; q < NV; ++q) v[q] += dpp_f<0x4E>(v[q]);
#pragma unroll
  for (int q = 0; q < NV; ++q) v[q] += dpp_f<0x141>(v[q]);
#pragma unroll
  for (int q = 0; q < NV; ++q) v[q] += dpp_f<0x140>(v[q]);
}

// tanh of the MLP activations (fc1, fc2, mean layer).  The split of Cephes
// tanhf: |x| < 0.625 an odd minimax polynomial, else 1 - 2/(e^{2|x|} + 1) on
// the hardware v_exp_f32 / v_rcp_f32; both arms straight-line, then a select.
// Within 2 ulp of the correctly rounded tanh over every f32 (GPU test
// test_tanh_f32_ulp, exhaustive), in ~15 VALU ops where the library tanhf's
// accurate exp and IEEE division take ~3x that.  Every MLP kernel (rollout
// policy/value, update rowpass) calls this one function, so logp_old from the
// rollout still equals the update's recomputation bit for bit.
__device__ __forceinline__ float tanh_small(float x) {                     // |x| < 0.625
  const float z = x * x;
  float p = fmaf(-5.70498872745e-3f, z, 2.06390887954e-2f);
  p = fmaf(p, z, -5.37397155531e-2f);
  p = fmaf(p, z, 1.33314422036e-1f);
  p = fmaf(p, z, -3.33332819422e-1f);
  return fmaf(p * z, x, x);
}
__device__ __forceinline__ float tanh_big(float x) {                       // the rest, NaN included
  const float e = __builtin_amdgcn_exp2f(fabsf(x) * 2.8853900817779268f); // e^{2|x|}; inf -> rcp 0 -> 1
  const float big = fmaf(-2.0f, __builtin_amdgcn_rcpf(e + 1.0f), 1.0f);
  return copysignf(big, x);
}
__device__ __forceinline__ float tanh_f32(float x) {
  const float small = tanh_small(x), big = tanh_big(x);
  return fabsf(x) < 0.625f ? small : big;                                 // NaN -> big arm -> NaN
}
// Where the two data-dependent short cuts are compiled in: where they measured
// faster in the regime that has them (raw-metre observations) and no slower
// with normalised ones -- the H 256 forward pass (tanh_f32_n on fc1) and the
// 32-row H 256 rowpass (phase E's zero test).  In the loss head, the
// column-split kernel and at H 64 / 128 both measured slower, with either kind
// of observation (EXPERIMENTS.md, "discarded tanh arms").
template <int H>
inline constexpr bool kTanhArms = H == 256;
template <int H, int R>
inline constexpr bool kZeroSkip = H == 256 && R == 32;
// The D skip (rowpass_kernel, "D skip"): phase E's zero test decided before
// phase D, whose product a saturated fc1 multiplies by zero.  In the k-packed
// kernel (both sync forms: the product's update step at H 256); the f32-rows
// instantiation of the same width (satrl_ppo_rowpass) is not on the product's
// path and keeps phase E's test alone.
template <int H, int R, bool KX>
inline constexpr bool kDSkip = kZeroSkip<H, R> && KX;

// tanh_f32 of the N values a call site holds, in place, with the arm chosen
// per wave: the MLP's activations are mostly of one kind over a whole wave --
// fc1 of raw-metre observations sits at |x| ~ 1e4, where every lane of
// tanh_f32 still paid for the polynomial it discards.  One compare-OR
// over the values and one ballot finds a wave with no small value (exp/rcp arm
// only); a second ballot, off that path, one with small values only
// (polynomial only); any other wave runs tanh_f32 as it is.  A lane's value
// goes through the arm tanh_f32 selects for it and the arms are the same
// instructions (no contraction: -ffp-contract=off), so every result bit is
// tanh_f32's (GPU test test_tanh_forms_bitwise).
template <int N>
__device__ __forceinline__ void tanh_f32_n(float (&v)[N]) {
  bool any_small = false;
#pragma unroll
  for (int q = 0; q < N; ++q) any_small |= fabsf(v[q]) < 0.625f;
  if (__builtin_amdgcn_ballot_w64(any_small) == 0) {
#pragma unroll
    for (int q = 0; q < N; ++q) v[q] = tanh_big(v[q]);
    return;
  }
  bool any_big = false;
#pragma unroll
  for (int q = 0; q < N; ++q) any_big |= !(fabsf(v[q]) < 0.625f);
  if (__builtin_amdgcn_ballot_w64(any_big) == 0) {
#pragma unroll
    for (int q = 0; q < N; ++q) v[q] = tanh_small(v[q]);
  } else {
#pragma unroll
    for (int q = 0; q < N; ++q) v[q] = tanh_f32(v[q]);
  }
}

// The k mapping of a 32-wide chunk (fc2 / dH1 phases): lane group g holds
// k = 8g + 4h + e, each lane's two float4 adjacent, so a wave-instruction
// touches every 128-B row segment at a 32-B stride (k = 16h + 4g + e, 64
// contiguous bytes per float4 instruction, measured no faster: EXPERIMENTS.md
// round 3).  Rollout and update share the mapping, hence the f32 rounding.
constexpr int kGOff = 8;   // floats between lane groups
constexpr int kHOff = 4;   // floats between a lane's two float4

template <int CT, int HOFF = kHOff>
__device__ __forceinline__ void b_chunk(const float* __restrict__ bp, int LDB, float4 (&b)[CT][2]) {
#pragma unroll
  for (int t = 0; t < CT; ++t) {
    b[t][0] = *reinterpret_cast<const float4*>(bp + 16 * t * LDB);
    b[t][1] = *reinterpret_cast<const float4*>(bp + 16 * t * LDB + HOFF);
  }
  __builtin_amdgcn_sched_barrier(0);   // keep the prefetch where it is issued
}

template <int LDA, int RT, int CT, int HOFF = kHOff>
__device__ __forceinline__ void mfma_chunk(const float* __restrict__ ap, const float4 (&b)[CT][2],
                                           f4 (&acc)[RT][CT]) {
  float4 a[RT][2];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    a[rt][0] = *reinterpret_cast<const float4*>(ap + 16 * rt * LDA);
    a[rt][1] = *reinterpret_cast<const float4*>(ap + 16 * rt * LDA + HOFF);
  }
#pragma unroll
  for (int h = 0; h < 2; ++h) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int t = 0; t < CT; ++t) acc[rt][t] = mfma4(a[rt][h][e], b[t][h][e], acc[rt][t]);
    }
  }
}

// the LDS A operand of one 32-wide k chunk, and the chunk's MFMAs on operands
// already in registers
template <int LDA, int RT>
__device__ __forceinline__ void a_chunk(const float* __restrict__ ap, float4 (&a)[RT][2]) {
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    a[rt][0] = *reinterpret_cast<const float4*>(ap + 16 * rt * LDA);
    a[rt][1] = *reinterpret_cast<const float4*>(ap + 16 * rt * LDA + kHOff);
  }
  __builtin_amdgcn_sched_barrier(0);
}
template <int RT, int CT>
__device__ __forceinline__ void mfma_regs(const float4 (&a)[RT][2], const float4 (&b)[CT][2], f4 (&acc)[RT][CT]) {
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int t = 0; t < CT; ++t) acc[rt][t] = mfma4(a[rt][h][e], b[t][h][e], acc[rt][t]);
}

// acc[rt][t] += A[16rt.. +16][K] (LDS, row stride LDA) x B^T with B[n][k]
// row-major (ld LDB) for columns n0 + 16t, in 32-wide k chunks.  Without
// APRE (the policy kernel): chunk pairs with two register buffers in a rolled
// loop (prefetch distance one chunk), loads unconditional and the last pair
// peeled, so every vmcnt wait is exact.  APRE (the rowpass): the LDS A chunk
// is double-buffered too, so a chunk's MFMAs do not start behind a fresh
// ds_read's latency (34.7 -> 33.6 us), and B runs kBPD chunks ahead.  Its
// registers are what the policy kernel's occupancy does not afford (54 VGPRs
// allow two 16-wave workgroups per CU; APRE: 59 -> 63 us per rollout step, B
// two ahead alone: 64 us).  The MFMA sequence, hence every result bit, is the
// same on every path.
// APRE path: B chunks kBPD ahead (kBPD + 1 register buffers; distance 2
// measured best: 30.7 us per rowpass against 32.5 at 1, 31.0 at 3, 31.7 at 4).
// The first kBPD chunks can be issued early, before the phase's barrier, into
// a WPre (mfma_rows_pre), and handed to mfma_rows<..., PRE = true> (phase D:
// 30.4 -> 29.8 us; the same for phase B measured no gain).
constexpr int kBPD = 2;
template <int CT>
struct WPre {
  float4 bb[kBPD][CT][2];
};
template <int LDB, int CT>
__device__ __forceinline__ void mfma_rows_pre(const float* __restrict__ B, int n0, WPre<CT>& pre) {
  const int l = threadIdx.x & 63, i = l & 15, g = l >> 4;
  const float* bp = B + (int64_t)(n0 + i) * LDB + kGOff * g;
  constexpr int BPD = kBPD < LDB / 32 ? kBPD : LDB / 32;      // (K = LDB here: W2 / W2T rows)
#pragma unroll
  for (int c = 0; c < BPD; ++c) b_chunk<CT>(bp + 32 * c, LDB, pre.bb[c]);
}

template <int K, int LDA, int LDB, int RT, int CT, bool APRE, bool PRE = false>
__device__ __forceinline__ void mfma_rows(const float* __restrict__ A, const float* __restrict__ B, int n0,
                                          f4 (&acc)[RT][CT], const WPre<CT>* pre = nullptr) {
  constexpr int NC = K / 32;
  constexpr int BPD = kBPD < NC ? kBPD : NC;                     // prefetch distance in chunks
  static_assert(NC % 2 == 0, "chunk pairs");
  static_assert(APRE || !PRE, "early-issued chunks feed the APRE path");
  const int l = threadIdx.x & 63, i = l & 15, g = l >> 4;
  const float* ap = A + i * LDA + kGOff * g;
  const float* bp = B + (int64_t)(n0 + i) * LDB + kGOff * g;
  if constexpr (APRE) {
    // fully unrolled so every buffer index is static
    constexpr int NB = BPD + 1;
    float4 bb[NB][CT][2], aa[2][RT][2];
    if constexpr (PRE) {
#pragma unroll
      for (int c = 0; c < BPD; ++c)
#pragma unroll
        for (int t = 0; t < CT; ++t) { bb[c][t][0] = pre->bb[c][t][0]; bb[c][t][1] = pre->bb[c][t][1]; }
    } else {
#pragma unroll
      for (int c = 0; c < BPD; ++c) b_chunk<CT>(bp + 32 * c, LDB, bb[c]);
    }
    a_chunk<LDA, RT>(ap, aa[0]);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      if (c + BPD < NC) b_chunk<CT>(bp + 32 * (c + BPD), LDB, bb[(c + BPD) % NB]);
      if (c + 1 < NC) a_chunk<LDA, RT>(ap + 32 * (c + 1), aa[(c + 1) % 2]);
      mfma_regs<RT, CT>(aa[c % 2], bb[c % NB], acc);
    }
  } else {
    float4 x[CT][2], y[CT][2];
    b_chunk<CT>(bp, LDB, x);
#pragma unroll 1
    for (int c = 0; c < NC - 2; c += 2) {
      b_chunk<CT>(bp + 32 * (c + 1), LDB, y);
      mfma_chunk<LDA, RT, CT>(ap + 32 * c, x, acc);
      b_chunk<CT>(bp + 32 * (c + 2), LDB, x);
      mfma_chunk<LDA, RT, CT>(ap + 32 * (c + 1), y, acc);
    }
    b_chunk<CT>(bp + 32 * (NC - 1), LDB, y);
    mfma_chunk<LDA, RT, CT>(ap + 32 * (NC - 2), x, acc);
    mfma_chunk<LDA, RT, CT>(ap + 32 * (NC - 1), y, acc);
  }
}

// ---------------------------------------------------------------------------
// fc2 products at H = 256 as three-way bf16 splits (kBf3): gfx950 has no
// reduced-precision f32 MFMA, and v_mfma_f32_16x16x4_f32 issues 2048 FLOP per
// 32 cycles where v_mfma_f32_16x16x32_bf16 issues 16384 per 16.  Every f32
// operand x is split x = hi + mid + lo exactly (round-to-nearest bf16 splits:
// each residual is exact in f32 and the last one fits bf16's 8 bits), and a
// product is the six partial products whose magnitude reaches f32's
// rounding (lo*hi, hi*lo, mid*mid, mid*hi, hi*mid, hi*hi, smallest first;
// the dropped mid*lo, lo*mid, lo*lo are below 2^-24 of it), each exact in the
// MFMA's f32 accumulator.  Measured (tools/bf16x3_probe.hip, K = 256): error
// / sum|a*b| max 2.2e-7, mean 1.3e-8 against 2.9e-7 / 1.7e-8 for the f32
// MFMA chain.  The A operand (activations, written once per row block) goes
// to LDS as three bf16 planes; the B operand (fc2.weight / its transpose,
// read once per workgroup from L2) stays f32 and is split in registers, 36
// VALU per 32-wide k chunk beside its 12 MFMAs.  The 16x16x32 operand layout
// (lane l: row / column l & 15, k = 8 (l >> 4) + j) is the f32 path's k
// mapping, and its accumulator layout the 16x16x4's, so nothing else changes.
// ---------------------------------------------------------------------------
template <int H>
inline constexpr bool kBf3 = H == 256;
typedef short s8v __attribute__((ext_vector_type(8)));   // 8 bf16: a 16x16x32 operand (4 VGPRs)

__device__ __forceinline__ unsigned short bf16_rne(float x) { return __builtin_bit_cast(unsigned short, (__bf16)x); }
__device__ __forceinline__ float bf16_up(unsigned short h) { return __uint_as_float((unsigned)h << 16); }
// x = hi + mid + lo exactly
__device__ __forceinline__ void split3(float x, unsigned short& h, unsigned short& m, unsigned short& l) {
  h = bf16_rne(x);
  const float r = x - bf16_up(h);
  m = bf16_rne(r);
  const float q = r - bf16_up(m);
  l = bf16_rne(q);
}
typedef float f2v __attribute__((ext_vector_type(2)));
typedef __bf16 bf2v __attribute__((ext_vector_type(2)));
typedef unsigned u4v __attribute__((ext_vector_type(4)));
// two f32 -> one dword of two bf16 (v_cvt_pk_bf16_f32, round to nearest even), and back
__device__ __forceinline__ unsigned pk_bf16(f2v x) { return __builtin_bit_cast(unsigned, __builtin_convertvector(x, bf2v)); }
__device__ __forceinline__ f2v unpk_bf16(unsigned p) {
  return f2v{__uint_as_float(p << 16), __uint_as_float(p & 0xffff0000u)};
}
// x - (the bf16 pair p, widened), per lane half, as one v_dot2c_f32_bf16 each
// (p . (-1, 0) + x.x and p . (0, -1) + x.y): the difference is exact in f32
// (p is x rounded to bf16), so the dot's single rounding returns it unchanged
// -- two VALU where widening p and a packed subtraction take three
// The (-1, 0) / (0, -1) operands go through SGPRs: the compiler encodes
// (-1, 0) as the inline constant -1.0, which the instruction reads as the f32
// pattern (0, -1) -- the wrong half (tools/dot2_exact.hip).
__device__ __forceinline__ bf2v sgpr_bf16x2(unsigned bits) {
  unsigned r;
  asm("s_mov_b32 %0, %1" : "=s"(r) : "i"(bits));
  return __builtin_bit_cast(bf2v, r);
}
__device__ __forceinline__ f2v resid_bf16(f2v x, unsigned p) {
  const bf2v pv = __builtin_bit_cast(bf2v, p);
  return f2v{__builtin_amdgcn_fdot2_f32_bf16(pv, sgpr_bf16x2(0x0000bf80u), x.x, false),
             __builtin_amdgcn_fdot2_f32_bf16(pv, sgpr_bf16x2(0xbf800000u), x.y, false)};
}
// split3 on a pair, packed: 7 VALU per pair (3 v_cvt_pk_bf16_f32, 4 v_dot2c_f32_bf16)
__device__ __forceinline__ void split3x2(f2v x, unsigned& h, unsigned& m, unsigned& l) {
  h = pk_bf16(x);
  const f2v r = resid_bf16(x, h);
  m = pk_bf16(r);
  const f2v q = resid_bf16(r, m);
  l = pk_bf16(q);
}
__device__ __forceinline__ void split3x8(const float4 (&x)[2], s8v (&o)[3]) {
  unsigned h[4], m[4], l[4];
  split3x2(f2v{x[0].x, x[0].y}, h[0], m[0], l[0]);
  split3x2(f2v{x[0].z, x[0].w}, h[1], m[1], l[1]);
  split3x2(f2v{x[1].x, x[1].y}, h[2], m[2], l[2]);
  split3x2(f2v{x[1].z, x[1].w}, h[3], m[3], l[3]);
  o[0] = __builtin_bit_cast(s8v, u4v{h[0], h[1], h[2], h[3]});
  o[1] = __builtin_bit_cast(s8v, u4v{m[0], m[1], m[2], m[3]});
  o[2] = __builtin_bit_cast(s8v, u4v{l[0], l[1], l[2], l[3]});
}
__device__ __forceinline__ f4 mfma_bf16(s8v a, s8v b, f4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
// the six partial products of one 16x16 tile and 32-wide k chunk, smallest first
__device__ __forceinline__ f4 mfma6(const s8v (&a)[3], const s8v (&bs)[3], f4 c) {
  c = mfma_bf16(a[2], bs[0], c);
  c = mfma_bf16(a[0], bs[2], c);
  c = mfma_bf16(a[1], bs[1], c);
  c = mfma_bf16(a[1], bs[0], c);
  c = mfma_bf16(a[0], bs[1], c);
  return mfma_bf16(a[0], bs[0], c);
}
// one 32-wide k chunk: A planes (registers) x B (f32, split here)
// BOR: *bor |= the raw f32 bits of every B element (two v_or3_b32 per float4;
// the rowpass's phase B, for its D skip).  The empty asm pins the ORs to the
// split that consumes the chunk: left to the scheduler they drift away from
// it, the raw chunks stay live, and the 32-row kernel went from 102 VGPRs to
// 128 and 84 B of scratch.
template <int RT, int CT, bool BOR = false>
__device__ __forceinline__ void mfma3_regs(const s8v (&a)[RT][3], const float4 (&b)[CT][2], f4 (&acc)[RT][CT],
                                           unsigned* bor = nullptr) {
#pragma unroll
  for (int t = 0; t < CT; ++t) {
    if constexpr (BOR) {
      unsigned o = *bor;
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        o |= __float_as_uint(b[t][q].x) | __float_as_uint(b[t][q].y);
        o |= __float_as_uint(b[t][q].z) | __float_as_uint(b[t][q].w);
      }
      asm volatile("" : "+v"(o));
      *bor = o;
    }
    s8v bs[3];
    split3x8(b[t], bs);
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) acc[rt][t] = mfma6(a[rt], bs, acc[rt][t]);
  }
}
template <int LDP, int PS, int RT>
__device__ __forceinline__ void a3_chunk(const unsigned short* __restrict__ ap, s8v (&a)[RT][3]) {
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int p = 0; p < 3; ++p) a[rt][p] = *reinterpret_cast<const s8v*>(ap + p * PS + 16 * rt * LDP);
  __builtin_amdgcn_sched_barrier(0);
}
// mfma_rows (APRE path) on the split operands: A = three bf16 planes in LDS
// (row stride LDP, plane stride PS elements), B f32 row-major (ld LDB) as
// there, kBPD chunks ahead, its first chunks optionally issued early (pre)
constexpr int kBPD3 = 2;          // B chunks in flight ahead of the MFMAs
constexpr int kADB3 = 1;          // A chunk buffers (2: the next chunk's LDS reads before this one's MFMAs: no faster)
// wait(c): called before the A operand reads of chunk c (the rowpass's
// hand-off form waits there for the waves that wrote the chunk's columns,
// RpHandoff below; NoChunkWait: the caller's barrier covers all of A)
struct NoChunkWait {
  __device__ __forceinline__ void operator()(int) const {}
};
// BOR: the OR of the B elements' bits goes into *bor (mfma3_regs)
template <int K, int LDP, int PS, int LDB, int RT, int CT, bool PRE = false, bool BOR = false,
          class Wait = NoChunkWait>
__device__ __forceinline__ void mfma_rows3(const unsigned short* __restrict__ A, const float* __restrict__ B, int n0,
                                           f4 (&acc)[RT][CT], const WPre<CT>* pre = nullptr, Wait wait = Wait(),
                                           unsigned* bor = nullptr) {
  constexpr int NC = K / 32;
  constexpr int BPD = kBPD3 < NC ? kBPD3 : NC, NB = BPD + 1;
  static_assert(!PRE || BPD >= kBPD, "early-issued chunks fit the ring");
  const int l = threadIdx.x & 63, i = l & 15, g = l >> 4;
  const unsigned short* ap = A + i * LDP + 8 * g;
  const float* bp = B + (int64_t)(n0 + i) * LDB + kGOff * g;
  float4 bb[NB][CT][2];
  s8v aa[kADB3][RT][3];
  if constexpr (PRE) {
#pragma unroll
    for (int c = 0; c < kBPD; ++c)
#pragma unroll
      for (int t = 0; t < CT; ++t) { bb[c][t][0] = pre->bb[c][t][0]; bb[c][t][1] = pre->bb[c][t][1]; }
#pragma unroll
    for (int c = kBPD; c < BPD; ++c) b_chunk<CT>(bp + 32 * c, LDB, bb[c]);
  } else {
#pragma unroll
    for (int c = 0; c < BPD; ++c) b_chunk<CT>(bp + 32 * c, LDB, bb[c]);
  }
  if constexpr (kADB3 == 2) {
    wait(0);
    a3_chunk<LDP, PS, RT>(ap, aa[0]);
  }
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    if (c + BPD < NC) b_chunk<CT>(bp + 32 * (c + BPD), LDB, bb[(c + BPD) % NB]);
    if constexpr (kADB3 == 2) {
      if (c + 1 < NC) {
        wait(c + 1);
        a3_chunk<LDP, PS, RT>(ap + 32 * (c + 1), aa[(c + 1) % 2]);
      }
    } else {
      wait(c);
      a3_chunk<LDP, PS, RT>(ap + 32 * c, aa[0]);
    }
    mfma3_regs<RT, CT, BOR>(aa[kADB3 == 2 ? c % 2 : 0], bb[c % NB], acc, bor);
  }
}

// ---------------------------------------------------------------------------
// The fc2 operand image W2X: the f32 W2^T [2][H][H] of both nets (phases D of
// the rowpass read fc2.weight transposed), written by adam_kernel beside each
// updated 32x32 tile and by satrl_ppo_w2x_sync from P.  A pre-split bf16
// planes image at H = 256 (no split VALU in the rowpass) was built and
// measured slower -- 1.5x the weight bytes from L2 (EXPERIMENTS.md round 4,
// commit e2546b9) -- so every width keeps the f32 image.
// ---------------------------------------------------------------------------
__host__ __device__ constexpr int64_t w2x_floats(int H) { return 2LL * H * H; }
// the three planes of 4 consecutive elements v (at e, plane stride PS) as
// three 8-B stores
__device__ __forceinline__ void put3x4(unsigned short* __restrict__ img, int64_t e, int64_t PS, float4 v) {
  unsigned h0, m0, l0, h1, m1, l1;
  split3x2(f2v{v.x, v.y}, h0, m0, l0);
  split3x2(f2v{v.z, v.w}, h1, m1, l1);
  *reinterpret_cast<uint2*>(img + e) = make_uint2(h0, h1);
  *reinterpret_cast<uint2*>(img + PS + e) = make_uint2(m0, m1);
  *reinterpret_cast<uint2*>(img + 2 * PS + e) = make_uint2(l0, l1);
}

// Row-parallel activations for the split-bf16 dW2 (satrl_ppo_rowpass_kx /
// satrl_ppo_dw2_kx): a [rows][H] f32 tensor of one net as three bf16 planes
// (plane stride PL elements), "k-packed": element (r, n) at ((r / 8) * H + n)
// * 8 + r % 8, so the 8 consecutive rows an MFMA operand lane holds (the
// reduction index of dW2 = dZ2^T H1 is the row) are one 16-B run, and the 16
// columns of a lane group one 256-B run.  A rowpass lane holds rows 4lg..4lg+3
// of a 16-row tile: one 8-B store per plane.
template <int H, int R, int CT>
__device__ __forceinline__ void store_kx(unsigned short* __restrict__ img, int64_t PL, int r0, int n0,
                                         const float (&v)[R / 16][CT][4]) {
  const int l = threadIdx.x & 63, li = l & 15, lg = l >> 4;
#pragma unroll
  for (int rt = 0; rt < R / 16; ++rt)
#pragma unroll
    for (int t = 0; t < CT; ++t) {
      const int r = r0 + 16 * rt + 4 * lg, n = n0 + 16 * t + li;
      put3x4(img, ((int64_t)(r >> 3) * H + n) * 8 + (r & 7), PL,
             make_float4(v[rt][t][0], v[rt][t][1], v[rt][t][2], v[rt][t][3]));
    }
}
// one 8-B store of the k-packed planes; WT: agent-scope write-through
// (global_store_dwordx2 sc0 sc1), so the planes leave L2 during the kernel
// instead of in the release at its end, which the next launch's start waits
// for.  The 16-row (short-minibatch) rowpass writes through: in-graph step at
// mb 512 33.1-33.2 against 34.1 us with plain stores (three alternations on
// two boxes, tools/ab_spans.sh); at mb 4096 the 32-row kernel gets as much
// longer as the boundary gets shorter (rowpass span +2-3 us, step equal), so
// it stores plainly (EXPERIMENTS.md round 6)
template <bool WT>
__device__ __forceinline__ void st_kx(unsigned short* p, uint2 v) {
  if constexpr (WT)
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), ((unsigned long long)v.y << 32) | v.x,
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else
    *reinterpret_cast<uint2*>(p) = v;
}

// store_kx from values already split (split3x2 of rows j, j+1 and j+2, j+3 of
// each lane's four; w[rt][t] = {hi01, hi23, mid01, mid23, lo01, lo23}): the
// same stores, no split VALU
template <int H, int R, int CT, bool WT = false>
__device__ __forceinline__ void store_kx_w(unsigned short* __restrict__ img, int64_t PL, int r0, int n0,
                                           const unsigned (&w)[R / 16][CT][6]) {
  const int l = threadIdx.x & 63, li = l & 15, lg = l >> 4;
#pragma unroll
  for (int rt = 0; rt < R / 16; ++rt)
#pragma unroll
    for (int t = 0; t < CT; ++t) {
      const int r = r0 + 16 * rt + 4 * lg, n = n0 + 16 * t + li;
      const int64_t e = ((int64_t)(r >> 3) * H + n) * 8 + (r & 7);
      st_kx<WT>(img + e, make_uint2(w[rt][t][0], w[rt][t][1]));
      st_kx<WT>(img + PL + e, make_uint2(w[rt][t][2], w[rt][t][3]));
      st_kx<WT>(img + 2 * PL + e, make_uint2(w[rt][t][4], w[rt][t][5]));
    }
}
// four values of one column, rows e, e + LDP, e + 2 LDP, e + 3 LDP of an LDS
// plane image (plane stride PS), split once as pairs (split3x2) into w: each
// bf16 goes out by a 16-bit store of its half of the packed word
// (ds_write_b16 / ds_write_b16_d16_hi), so the planes get the bits put3 gives
// each value, with the split VALU of two pairs instead of four scalars
template <int PS, int LDP>
__device__ __forceinline__ void put3_col4(unsigned short* img, int e, const float (&v)[4], unsigned (&w)[6]) {
  split3x2(f2v{v[0], v[1]}, w[0], w[2], w[4]);
  split3x2(f2v{v[2], v[3]}, w[1], w[3], w[5]);
#pragma unroll
  for (int p = 0; p < 3; ++p) {
    img[p * PS + e] = (unsigned short)w[2 * p];
    img[p * PS + e + LDP] = (unsigned short)(w[2 * p] >> 16);
    img[p * PS + e + 2 * LDP] = (unsigned short)w[2 * p + 1];
    img[p * PS + e + 3 * LDP] = (unsigned short)(w[2 * p + 1] >> 16);
  }
}
// rows of a k-packed tensor: the minibatch padded to whole 32-row chunks
__host__ __device__ constexpr int64_t kx_rows(int mb) { return (mb + 31) / 32 * 32LL; }
// the three planes of x at element e of an LDS plane image (plane stride PS)
template <int PS>
__device__ __forceinline__ void put3(unsigned short* img, int e, float x) {
  unsigned short h, m, l;
  split3(x, h, m, l);
  img[e] = h;
  img[PS + e] = m;
  img[2 * PS + e] = l;
}

// rows r < nvalid of a 32-/16-row block's accumulator-layout values v[rt][t][j]
// (row 16rt + 4lg + j, column n0 + 16t + li) to out[r * ld + column]: a
// uniform branch keeps a full block's stores straight-line (a per-lane test
// made every store its own exec-masked branch)
template <int R, int CT>
__device__ __forceinline__ void store_rows(float* __restrict__ out, int ld, int n0, int nvalid,
                                           const float (&v)[R / 16][CT][4]) {
  const int l = threadIdx.x & 63, li = l & 15, lg = l >> 4;
  if (nvalid >= R) {
#pragma unroll
    for (int rt = 0; rt < R / 16; ++rt)
#pragma unroll
      for (int t = 0; t < CT; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) out[(int64_t)(16 * rt + 4 * lg + j) * ld + n0 + 16 * t + li] = v[rt][t][j];
  } else {
#pragma unroll
    for (int rt = 0; rt < R / 16; ++rt)
#pragma unroll
      for (int t = 0; t < CT; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int r = 16 * rt + 4 * lg + j;
          if (r < nvalid) out[(int64_t)r * ld + n0 + 16 * t + li] = v[rt][t][j];
        }
  }
}

// Workgroup barrier of the MLP kernels' phases (__syncthreads: LDS-only
// barriers that leave the global stores and early weight chunks in flight
// measured no faster, EXPERIMENTS.md round 3).
__device__ __forceinline__ void rp_barrier() { __syncthreads(); }

// the rowpass error word (word 0): a column-split exchange (rowpass_cs_kernel)
// or an LDS hand-off (RpHandoff) that ran out of its wait;
// satrl_ppo_rowpass_error reports and clears it
__device__ __attribute__((aligned(128))) unsigned g_cs_err[32];

// ---------------------------------------------------------------------------
// How the phases of a rowpass workgroup wait for each other: a template
// parameter (Sync) of the shared phase functions, two forms.
//
// RpBarrier: a workgroup barrier (rp_barrier) between the phases.  Every MLP
// kernel but the one below, and that kernel's own other instantiation.
//
// RpHandoff (the 32-row 16-wave H 256 k-packed rowpass): the barriers after
// the gather's are replaced by the dependencies the data really has, as LDS
// words (RpFlags) that a producer sets once its own LDS writes have landed
// (s_waitcnt lgkmcnt(0), then one lane's LDS atomic) and a consumer polls
// (one lane's ds_read, s_sleep between reads):
//   h1   bit w: wave w's columns of the H1 planes (phase A).  Phase B's
//        chunk c reads H1 columns 32c .. 32c+31 only: it waits for bits 2c
//        and 2c+1, so the oldest waves of a SIMD start B while its youngest
//        are still in fc1.
//   out  count: waves whose output-layer partials are in osum (and, from the
//        last wave, the head's constants).  Only wave 0 (the loss head)
//        waits for all NW.
//   dz3  wave 0's dz3s are written (the loss head is done): every other
//        wave waits for it before its tail.
//   dz   bit w: wave w's columns of the dZ2 planes (the tail); phase D's
//        chunk c waits for bits 2c and 2c+1.
// One word holds the 16 bits of h1 (of dz), so a wave that finds every bit
// set on its first read reads no flag again.  Thread 0 zeroes the words before
// the gather's barrier, which stays; each is used once per launch, so there
// are no epochs and nothing carries over from launch to launch.
// Dependency order, a DAG over (phase, wave) after the gather's barrier:
//   A(w) -> B(v) chunk w/2, every v;  B(w) -> out(w);  out(all) -> head (wave 0);
//   head -> tail(w), every w;  tail(w) -> D(v) chunk w/2, every v;  D(w) -> E(w);
//   tail(all) -> decision(w) of a wave w that may skip D (rowpass_kernel, "D
//   skip"): it waits for every dz bit, then runs D and E or neither.
// A producer step (A, out, head, tail) waits only for steps to its left, never
// for a consumer (none waits for a D or a decision), and all NW waves of a
// workgroup are resident together, so
// every wait ends.  No global-memory hand-off, no wait on another workgroup,
// no wait on vmcnt: the plane stores and early weight chunks stay in flight.
// Every poll is bounded (kRpPollMax sleeps, tens of ms): on running out the
// wave sets the rowpass error word and goes on, so a wrong flag ends as a
// reported error (satrl_ppo_rowpass_error), never as a hang.
// The arithmetic, the chunk and MFMA order and every operand are the barrier
// form's: every output bit is the same.
// ---------------------------------------------------------------------------
// wmag, dzmag (the D skip of the 32-row kernel, both sync forms): the OR of
// the raw f32 bits of every fc2.weight element the workgroup's waves load in
// phase B (together the net's whole fc2), and of every dZ2 value of the block.
// A wave ORs its share in (rp_or_put) just before it publishes out / dz (or
// arrives at the barrier that stands for them), so whoever has seen all of
// out (of dz) reads the complete word.
struct RpFlags {
  unsigned h1, dz, out, dz3, wmag, dzmag;
};
__device__ __forceinline__ void rp_flags_zero(RpFlags& f) {
  if (threadIdx.x == 0) f = RpFlags{0u, 0u, 0u, 0u, 0u, 0u};
}
__device__ __forceinline__ unsigned rp_wave() { return __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); }
// OR over the wave's 64 lanes, wave-uniform: DPP ORs along each 16-lane row
// (row16_sum's permutations), then the four rows' first lanes
__device__ __forceinline__ unsigned wave_or(unsigned v) {
  v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false);
  v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false);
  v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, false);
  v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, false);
  return (unsigned)(__builtin_amdgcn_readlane((int)v, 0) | __builtin_amdgcn_readlane((int)v, 16) |
                    __builtin_amdgcn_readlane((int)v, 32) | __builtin_amdgcn_readlane((int)v, 48));
}
// the wave's OR of v into an RpFlags magnitude word: lane 0's LDS atomic
__device__ __forceinline__ void rp_or_put(unsigned* word, unsigned v) {
  const unsigned o = wave_or(v);
  if ((threadIdx.x & 63) == 0) __hip_atomic_fetch_or(word, o, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
constexpr unsigned kRpPollMax = 1u << 19;

// this wave's LDS writes have landed; then lane 0's LDS atomic (OR: a bit, else add 1)
template <bool OR>
__device__ __forceinline__ void rp_publish(unsigned* word, unsigned v) {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  if ((threadIdx.x & 63) == 0) {
    if constexpr (OR) __hip_atomic_fetch_or(word, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else __hip_atomic_fetch_add(word, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
}
__device__ __forceinline__ unsigned rp_read(const unsigned* word) {
  unsigned v = 0;
  if ((threadIdx.x & 63) == 0) v = __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  return __builtin_amdgcn_readfirstlane(v);
}
// waits until (word & mask) == mask (word >= mask: a count, with GE); returns the word
template <bool GE = false>
__device__ __forceinline__ unsigned rp_wait(const unsigned* word, unsigned mask) {
  unsigned v = rp_read(word);
#pragma nounroll
  for (unsigned it = 0; GE ? v < mask : (v & mask) != mask; ++it) {
    if (it == kRpPollMax) {
      if ((threadIdx.x & 63) == 0) __hip_atomic_store(&g_cs_err[0], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      break;
    }
    __builtin_amdgcn_s_sleep(1);
    v = rp_read(word);
  }
  asm volatile("" ::: "memory");                                   // the payload's LDS reads stay behind the poll
  return v;
}

// (the stamp numbers of the two forms agree: 1, 4, 5 = the wave passed the
// wait -- in the hand-off form its first chunk's)
struct RpBarrier {
  static constexpr bool kHandoff = false;
  __device__ __forceinline__ void init() {}
  __device__ __forceinline__ void after_gather() {}
  __device__ __forceinline__ void h1_written() { rp_barrier(); PHASE_PROBE(1); }
  __device__ __forceinline__ void out_written() { rp_barrier(); }
  __device__ __forceinline__ void wait_out() {}
  __device__ __forceinline__ void head_done() { rp_barrier(); PHASE_PROBE(4); }
  __device__ __forceinline__ void dz_written() { rp_barrier(); PHASE_PROBE(5); }
  __device__ __forceinline__ NoChunkWait wait_h1() { return NoChunkWait(); }
  __device__ __forceinline__ NoChunkWait wait_dz() { return NoChunkWait(); }
};
// RpBarrier of a kernel that keeps the magnitude words (the D skip)
struct RpBarrierMag : RpBarrier {
  RpFlags& f;
  __device__ __forceinline__ explicit RpBarrierMag(RpFlags& flags) : f(flags) {}
  __device__ __forceinline__ void init() { rp_flags_zero(f); }
};
template <int NW, class Head>
struct RpHandoff {
  static constexpr bool kHandoff = true;
  static_assert(NW == 16, "a 32-column chunk is two waves' tiles; 16 bits per word");
  RpFlags& f;
  Head head;                                                        // the head's constants (head_consts)
  __device__ __forceinline__ void init() { rp_flags_zero(f); }
  __device__ __forceinline__ void after_gather() { head(); }
  __device__ __forceinline__ void h1_written() { rp_publish<true>(&f.h1, 1u << rp_wave()); }
  __device__ __forceinline__ void out_written() { rp_publish<false>(&f.out, 1u); }
  __device__ __forceinline__ void wait_out() {
    if (threadIdx.x < 64) rp_wait<true>(&f.out, (unsigned)NW);
  }
  __device__ __forceinline__ void head_done() {
    if (threadIdx.x < 64) rp_publish<false>(&f.dz3, 1u);
    else rp_wait<true>(&f.dz3, 1u);
    PHASE_PROBE(4);
  }
  __device__ __forceinline__ void dz_written() { rp_publish<true>(&f.dz, 1u << rp_wave()); }
  // before the A operand reads of chunk c: the two waves that wrote its columns
  template <int STAMP>
  struct ChunkWait {
    const unsigned* word;
    unsigned seen;
    __device__ __forceinline__ void operator()(int c) {
      const unsigned m = 3u << (2 * c);
      if ((seen & m) != m) seen = rp_wait(word, m);
      if (c == 0) PHASE_PROBE(STAMP);
    }
  };
  __device__ __forceinline__ ChunkWait<1> wait_h1() { return ChunkWait<1>{&f.h1, 0u}; }
  __device__ __forceinline__ ChunkWait<5> wait_dz() { return ChunkWait<5>{&f.dz, 0u}; }
};
template <int NW, class Head>
__device__ __forceinline__ RpHandoff<NW, Head> rp_handoff(RpFlags& f, Head head) {
  return RpHandoff<NW, Head>{f, head};
}

// ---------------------------------------------------------------------------
// The phases that rowpass_kernel (its forward part through mlp_forward) and
// the column-split rowpass_cs_kernel both run, written once: the column-split
// kernel is the RT = CT = 1, R = kRowsShort instantiation, so its values are
// the 16-wave kernel's by construction.  The two kernels lay their shared
// memory out differently, so every LDS array comes as a reference.
// n0: the first hidden column of the wave's tiles.
// ---------------------------------------------------------------------------
// The head's scalars (mean_layer bias, log_std, fc3 bias) and its
// per-dimension constants (var = exp(log_std)^2, log std, 1/var), off the
// head's dependency chain: lanes 0-3 of the last wave (no row load of its
// own at H = 256) load them as per-lane vector loads (head_load, at the top of
// the kernel) and compute the constants into LDS during the gather
// (head_consts; the barriers of the forward pass publish them).  Uniform
// scalar loads of P here would make the wave's first s_waitcnt lgkmcnt -- the
// one for the kernel arguments -- wait for them before any row load is issued.
template <int H, int NT>
__device__ __forceinline__ void head_load(const float* __restrict__ P, float& hls_d, float& hb3_d) {
  const Layout L = layout(H);
  const int hd = (int)threadIdx.x - (NT - 64);                     // head-scalar lane of the last wave
  hls_d = 0.0f;
  hb3_d = 0.0f;
  if (hd >= 0 && hd < 4) {
    hb3_d = P[hd < 3 ? L.b3a + hd : L.b3c];
    hls_d = P[L.ls + (hd < 3 ? hd : 0)];
  }
}
template <int NT>
__device__ __forceinline__ void head_consts(float& hls_d, float& hb3_d, float (&hcs)[3][3], float (&hb3s)[4]) {
  // (opaque to the compiler and ordered after the row loads: otherwise it
  // hoists this arithmetic next to its loads at the top of the kernel,
  // and the whole wave waits for them before issuing any row load)
  asm volatile("" : "+v"(hls_d), "+v"(hb3_d)::"memory");
  const int hd = (int)threadIdx.x - (NT - 64);
  if (hd >= 0 && hd < 4) {
    hb3s[hd] = hb3_d;                                               // b3a[0..2], b3c
    if (hd < 3) {
      const float sd = expf(hls_d), var = sd * sd;
      hcs[0][hd] = var;
      hcs[1][hd] = logf(sd);
      hcs[2][hd] = 1.0f / var;
    }
  }
}

// rows r0 .. r0 + R of the minibatch (staged: src rows; else src[idx[row]])
// -> S (the state) and ax (a, logp_old, adv, v_target), thread t0 of nt; the
// head's constants on the way (HEADC; the hand-off rowpass computes them
// after the gather's barrier instead, RpHandoff::after_gather).  Returns
// whether every state value this thread put into S is finite (phase E's guard).
template <int R, int NT, bool HEADC = true, int LDS_S>
__device__ __forceinline__ bool gather_rows(int mb, const float* __restrict__ src, const int64_t* __restrict__ idx,
                                            int r0, int t0, int nt, float (&S)[R][LDS_S], float (&ax)[R][8],
                                            float& hls_d, float& hb3_d, float (&hcs)[3][3], float (&hb3s)[4]) {
  bool fin = true;
  if (idx == nullptr) {
    // contiguous (staged) rows: one 16-B load per thread covers the block's
    // R x 32 floats, all in flight at once (a loop of dependent scalar
    // loads took four load round trips at H = 64's 256 threads)
    // (branch-free: rows past the minibatch load its last row, zeroed below)
    static_assert(R * 8 <= NT, "one float4 per thread");
    const int r = (t0 >> 3) & (R - 1), c4 = t0 & 7, row = r0 + r;
    const bool in = t0 < R * 8;
    float4 v = reinterpret_cast<const float4*>(src)[(int64_t)(row < mb ? row : mb - 1) * 8 + c4];
    if constexpr (HEADC) head_consts<NT>(hls_d, hb3_d, hcs, hb3s);
    if (row >= mb) v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (in) {
      const float e4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = 4 * c4 + e;                                  // s | a, logp_old, adv, v_target | pad
        if (c < 18) {
          S[r][c] = e4[e];
          fin &= __builtin_isfinite(e4[e]);
        } else if (c < 26) {
          ax[r][c - 18] = e4[e];
        }
      }
    }
  } else {
    for (int q = t0; q < R * 26; q += nt) {
      const int r = q / 26, c = q % 26, row = r0 + r;
      const float v = row < mb ? src[idx[row] * 32 + c] : 0.0f;
      if (c < 18) {
        S[r][c] = v;
        fin &= __builtin_isfinite(v);
      } else {
        ax[r][c - 18] = v;
      }
    }
    if constexpr (HEADC) head_consts<NT>(hls_d, hb3_d, hcs, hb3s);
  }
  return fin;
}
// the guard's publication: word w of nfw says whether wave w gathered a
// non-finite state value.  Every wave writes its own word before the gather's
// barrier (nothing to zero first); phase E reads all of them.
__device__ __forceinline__ void rows_finite_put(unsigned* nfw, bool fin) {
  const unsigned long long bad = __builtin_amdgcn_ballot_w64(!fin);
  if ((threadIdx.x & 63) == 0) nfw[threadIdx.x >> 6] = bad != 0 ? 1u : 0u;
}

// columns 18.. of S: the bias column of W1aug (rows of the minibatch), zero pad
template <int NT, int R, int LDS_S>
__device__ __forceinline__ void pad_rows(float (&S)[R][LDS_S], int nvalid) {
  for (int q = threadIdx.x; q < R * (LDS_S - 18); q += NT) {
    const int r = q / (LDS_S - 18), c = 18 + q % (LDS_S - 18);
    S[r][c] = (c == 18 && r < nvalid) ? 1.0f : 0.0f;
  }
}

// acc = tanh(acc + fc2 bias) for a wave's CT column tiles, and the tiles'
// output-layer partials -> part[row][output][tile0 + t].  li, lg: the lane's
// l & 15 and l >> 4, from the caller (recomputed here, the compiler no longer
// shares the forward pass's address arithmetic: the policy kernels' register
// counts moved).  One partial per
// 16-column tile (DPP row sums), so the output layer sums the same H/16
// partials in the same order whatever the wave count: the 8-wave policy
// kernel's log-probs are the 16-wave rowpass's bit for bit
template <int RT, int CT, int LD>
__device__ __forceinline__ void fc2_out_partials(f4 (&acc)[RT][CT], const float (&b2v)[CT], const float (&w3)[CT][3],
                                                 int net, int li, int lg, float (&part)[16 * RT][3][LD], int tile0) {
  const int NQ = net == 0 ? 3 : 1;                                  // output columns of this net
  float p[3][CT][RT][4];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int t = 0; t < CT; ++t)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float h = tanh_f32(acc[rt][t][j] + b2v[t]);           // fc2 + tanh
        acc[rt][t][j] = h;
#pragma unroll
        for (int q = 0; q < 3; ++q) p[q][t][rt][j] = fmaf(h, w3[t][q], 0.0f);
      }
  // the DPP row sums; NQ is uniform per workgroup (3 actor, 1 critic)
  constexpr int NP = CT * RT * 4;                                   // partials per output column
  float ps[3 * NP];
#pragma unroll
  for (int q = 0; q < 3; ++q)
#pragma unroll
    for (int t = 0; t < CT; ++t)
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int j = 0; j < 4; ++j) ps[((q * CT + t) * RT + rt) * 4 + j] = p[q][t][rt][j];
  if (NQ == 3) {
    row16_sum_n<3 * NP>(ps);
  } else {
    float p0[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) p0[k] = ps[k];
    row16_sum_n<NP>(p0);
#pragma unroll
    for (int k = 0; k < NP; ++k) ps[k] = p0[k];
  }
  if (li == 0) {
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      if (q >= NQ) break;
#pragma unroll
      for (int t = 0; t < CT; ++t)
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            part[16 * rt + 4 * lg + j][q][tile0 + t] = ps[((q * CT + t) * RT + rt) * 4 + j];
    }
  }
}

// output-layer pre-activation of row r, column d: the NTL column-tile
// partials in fixed order
template <int NTL, int OSP>
__device__ __forceinline__ float out_sum(const float (*osum)[3][OSP], int r, int d) {
  float od = 0.0f;
#pragma unroll
  for (int k = 0; k < NTL; ++k) od += osum[r][d][k];
  return od;
}

// The net's loss and its gradient for the block's R rows (threads 0 .. R-1,
// in wave 0): dz3s[r] = d loss / d (output-layer pre-activations), and, where
// `store`, the block's b3a / log_std / b3c partials to its tail slab tp and
// the actor's per-row ratio to ratio_out (nullable).  STAMP: phase stamps
// 12-14 (the probe build of rowpass_kernel).
template <int H, int R, bool STAMP, int OSP>
__device__ __forceinline__ void loss_head(int mb, int r0, int net, float inv_mb, float epsilon, float ent_coef,
                                          float max_action, const float (&osum)[R][3][OSP],
                                          const float (&hcs)[3][3], const float (&hb3s)[4], const float (&ax)[R][8],
                                          float (&dz3s)[R][4], float* tp, float* ratio_out, bool store) {
  const int r = threadIdx.x, row = r0 + r;
  if (r >= R) return;
  float dz[4] = {0.f, 0.f, 0.f, 0.f}, dls[4] = {0.f, 0.f, 0.f, 0.f};
  if (row < mb) {
    const float inv = inv_mb;                                     // 1.0f / (float)mb, IEEE on the host
    if (net == 0) {                                                // actor: clipped surrogate + entropy
      float th[3], mu[3], dv[3], var[3], logp[3];
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        th[d] = tanh_f32(out_sum<H / 16>(osum, r, d) + hb3s[d]);
        mu[d] = max_action * th[d];                                // 1.6 * tanh(mean_layer)
        var[d] = hcs[0][d];
        dv[d] = ax[r][d] - mu[d];
        // (the forward expression of gaussian_act, bit for bit: logp_old)
        logp[d] = (-(dv[d] * dv[d]) / (2.0f * var[d]) - hcs[1][d]) - kLogSqrt2Pi;
      }
      if constexpr (STAMP) PHASE_PROBE(12);
      const float lsum = (logp[0] + logp[1]) + logp[2];
      const float lold = (ax[r][3] + ax[r][4]) + ax[r][5];
      const float ratio = expf(lsum - lold);
      if (ratio_out != nullptr && store) ratio_out[row] = ratio;   // (satrl_ppo_rowpass_ratio)
      const float adv = ax[r][6];
      const float s1 = ratio * adv;
      const float cr = fminf(fmaxf(ratio, 1.0f - epsilon), 1.0f + epsilon);
      const float s2 = cr * adv;
      const float g1 = s1 < s2 ? 1.0f : (s1 == s2 ? 0.5f : 0.0f);   // torch.min tie split
      const float g2 = s2 < s1 ? 1.0f : (s1 == s2 ? 0.5f : 0.0f);
      const float inside = (ratio >= 1.0f - epsilon && ratio <= 1.0f + epsilon) ? 1.0f : 0.0f;
      const float dmin = -inv;
      const float dratio = dmin * g1 * adv + dmin * g2 * adv * inside;
      const float dlsum = dratio * ratio;
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        const float dvv = dv[d] * hcs[2][d];                       // (x - mu) / var
        const float dmu = dlsum * dvv;
        dz[d] = (dmu * max_action) * (1.0f - th[d] * th[d]);
        dls[d] = dlsum * (dv[d] * dvv - 1.0f) - ent_coef * inv;
      }
    } else {                                                       // critic: MSE
      const float vc = out_sum<H / 16>(osum, r, 0) + hb3s[3];
      dz[3] = 2.0f * inv * (vc - ax[r][7]);                        // d mse / d v
    }
  }
  if constexpr (STAMP) PHASE_PROBE(13);
#pragma unroll
  for (int q = 0; q < 4; ++q) dz3s[r][q] = dz[q];
  // the block's b3a / log_std / b3c partials: sums over its R rows, reduced
  // across these R lanes of wave 0 in a fixed order: DPP sums of each
  // 16-lane row, then row 0 + row 1 (readlane), no LDS round trips
  static_assert(R == 16 || R == 32, "row sums cover one or two DPP rows");
  float red[7] = {dz[0], dz[1], dz[2], dls[0], dls[1], dls[2], dz[3]};
  row16_sum_n<7>(red);
  if (R == 32) {
#pragma unroll
    for (int q = 0; q < 7; ++q)
      red[q] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(red[q]), 0)) +
               __int_as_float(__builtin_amdgcn_readlane(__float_as_int(red[q]), 16));
  }
  if constexpr (STAMP) PHASE_PROBE(14);
  if (r == 0 && store) {
    if (net == 0) {
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        tp[5 * H + q] = red[q];          // b3a
        tp[5 * H + 4 + q] = red[3 + q];  // log_std
      }
      tp[5 * H + 3] = 0.0f;
      tp[5 * H + 7] = 0.0f;
    } else {
      tp[6 * H + 8] = red[6];            // b3c
      tp[6 * H + 9] = 0.0f; tp[6 * H + 10] = 0.0f; tp[6 * H + 11] = 0.0f;
    }
  }
}

// The tail of phase C for a wave's CT column tiles at n0: dZ2 = (dz3s W3)
// (1 - tanh(fc2)^2) -> d2v, its LDS image (f32 rows dzs, or at the split-bf16
// width the planes dzp -- row stride LDP, plane stride PS -- with the split
// words kept in d2w), and the block's db2 /
// dW3 partials -> the tail slab tp.  Unswitched on the (workgroup-uniform)
// net: no per-element branches, and the critic skips the actor's three
// output columns.  (Moving the db2 / dW3 partial sums into phase D's MFMA gaps
// measured slower: D +2.6 k cycles for 0.5 k saved here, EXPERIMENTS.md
// round 4.)
template <int H, int RT, int CT, int LDP, int PS, bool ACT>
__device__ __forceinline__ void tail_net(const f4 (&acc)[RT][CT], const float (&w3)[CT][3],
                                         const float (&dz3s)[16 * RT][4], float* dzs, unsigned short* dzp,
                                         float (&d2v)[RT][CT][4], unsigned (&d2w)[RT][CT][6], float* tp,
                                         int net, int n0) {
  const int l = threadIdx.x & 63, li = l & 15, lg = l >> 4;
  constexpr bool BF3 = kBf3<H>;
  constexpr int LDA = H + 4;                                       // row stride of dzs
  constexpr int NC = ACT ? 3 : 1;
#pragma unroll
  for (int t = 0; t < CT; ++t) {
    const int n = n0 + 16 * t + li;
    float cb2 = 0.f, cw[NC];
#pragma unroll
    for (int q = 0; q < NC; ++q) cw[q] = 0.f;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = 16 * rt + 4 * lg + j;
        const float h = acc[rt][t][j];
        float dh;
        if constexpr (ACT) dh = (dz3s[r][0] * w3[t][0] + dz3s[r][1] * w3[t][1]) + dz3s[r][2] * w3[t][2];
        else dh = dz3s[r][3] * w3[t][0];
        const float d2 = dh * (1.0f - h * h);                     // tanh backward
        if constexpr (!BF3) dzs[r * LDA + n] = d2;
        d2v[rt][t][j] = d2;
        cb2 += d2;
        if constexpr (ACT) {
          cw[0] = fmaf(dz3s[r][0], h, cw[0]); cw[1] = fmaf(dz3s[r][1], h, cw[1]); cw[2] = fmaf(dz3s[r][2], h, cw[2]);
        } else {
          cw[0] = fmaf(dz3s[r][3], h, cw[0]);
        }
      }
      // (split-bf16) dZ2's LDS planes (phase D's A operand), split once as
      // pairs; the words stay in d2w for the k-packed dZ2 store
      if constexpr (BF3) put3_col4<PS, LDP>(dzp, (16 * rt + 4 * lg) * LDP + n, d2v[rt][t], d2w[rt][t]);
    }
    cb2 = xor32_sum(xor16_sum(cb2));
#pragma unroll
    for (int q = 0; q < NC; ++q) cw[q] = xor32_sum(xor16_sum(cw[q]));
    if (lg == 0) {
      tp[net * H + n] = cb2;                                     // db2
      if constexpr (ACT) {                                       // dW3a
        tp[2 * H + n] = cw[0]; tp[3 * H + n] = cw[1]; tp[4 * H + n] = cw[2];
      } else {
        tp[5 * H + 8 + n] = cw[0];                               // dW3c
      }
    }
  }
}
template <int H, int RT, int CT, int LDP, int PS>
__device__ __forceinline__ void tail(const f4 (&acc)[RT][CT], const float (&w3)[CT][3],
                                     const float (&dz3s)[16 * RT][4], float* dzs, unsigned short* dzp,
                                     float (&d2v)[RT][CT][4], unsigned (&d2w)[RT][CT][6], float* tp,
                                     int net, int n0) {
  if (net == 0) tail_net<H, RT, CT, LDP, PS, true>(acc, w3, dz3s, dzs, dzp, d2v, d2w, tp, net, n0);
  else tail_net<H, RT, CT, LDP, PS, false>(acc, w3, dz3s, dzs, dzp, d2v, d2w, tp, net, n0);
}

// Phase E for a wave's CT column tiles at n0: dZ1 = dH1 (1 - H1^2) in place,
// then [dW1 | db1][n][k'] = sum_r dZ1[r][n] S[r][k'] -> pw.
// acc[rt][t][j] = dZ1[row 16rt+4lg+j][n0+16t+li] is the A operand A[n][r] of
// the product (k = row, kk = j); B[r][k'] = S[16rt+4lg+kk][16hb + li] from LDS.
// Where fc1 is saturated (raw-metre observations: H1 = +-1 exactly) dZ1 is
// +-0 in every lane, and the MFMAs -- the last thing on the workgroup's path --
// only add +-0 x S to a +0 accumulator: +0 bits whenever S is finite.  So a
// wave whose dZ1 values are all +-0 (one OR and one ballot), in a block whose
// gathered rows are all finite (nfw, rows_finite_put: read only by such a
// wave), stores +0.0 and skips them; 0 x inf / 0 x NaN keep the MFMA path and
// its NaNs.
// SKIP: the kernels that take the short cut (kZeroSkip), nfw their NFW words.
// (phase_e_zero: the short cut's stores, +0.0 to the wave's [dW1|db1] slab
// rows; rows_finite_all: the guard.  Both also serve the D skip, which
// decides the same before phase D, rowpass_kernel.)
template <int CT>
__device__ __forceinline__ void phase_e_zero(float* pw, int n0) {
  const int l = threadIdx.x & 63, li = l & 15, lg = l >> 4;
#pragma unroll
  for (int t = 0; t < CT; ++t)
#pragma unroll
    for (int hb = 0; hb < 2; ++hb) {
      const int kp = 16 * hb + li;
      if (kp < 20) {
#pragma unroll
        for (int j = 0; j < 4; ++j) pw[(int64_t)(n0 + 16 * t + 4 * lg + j) * 20 + kp] = 0.0f;
      }
    }
}
// whether no wave of the block gathered a non-finite state value (wave-uniform)
template <int NFW>
__device__ __forceinline__ bool rows_finite_all(const unsigned* nfw) {
  return __builtin_amdgcn_ballot_w64(nfw[threadIdx.x & 63 & (NFW - 1)] != 0u) == 0;
}
template <bool SKIP, int NFW, int RT, int CT, int LDS_S>
__device__ __forceinline__ void phase_e(f4 (&acc)[RT][CT], const float (&h1)[RT][CT][4],
                                        const float (&S)[16 * RT][LDS_S], float* pw, int n0,
                                        const unsigned* nfw) {
  const int l = threadIdx.x & 63, li = l & 15, lg = l >> 4;
  unsigned nz = 0u;
#pragma unroll
  for (int t = 0; t < CT; ++t)
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        acc[rt][t][j] = acc[rt][t][j] * (1.0f - h1[rt][t][j] * h1[rt][t][j]);
        nz |= __float_as_uint(acc[rt][t][j]);
      }
  if (SKIP && __builtin_amdgcn_ballot_w64((nz & 0x7fffffffu) != 0u) == 0 && rows_finite_all<NFW>(nfw)) {
    phase_e_zero<CT>(pw, n0);
    return;
  }
#pragma unroll
  for (int t = 0; t < CT; ++t) {
#pragma unroll
    for (int hb = 0; hb < 2; ++hb) {
      f4 d = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) d = mfma4(acc[rt][t][kk], S[16 * rt + 4 * lg + kk][16 * hb + li], d);
      // d[j] = dW1aug[n = n0 + 16t + 4lg + j][k' = 16hb + li]
      const int kp = 16 * hb + li;
      if (kp < 20) {
#pragma unroll
        for (int j = 0; j < 4; ++j) pw[(int64_t)(n0 + 16 * t + 4 * lg + j) * 20 + kp] = d[j];
      }
    }
  }
}

// (k-packed) a wave's tiles of the block's H1 planes, from the split words
// h1w, and the zero rows of the padded 32-row chunk past a 16-row kernel's
// last block, in H1 and dZ2 (rows past the minibatch: zero inputs, so
// tanh(fc1) = 0 and dZ2 = 0 there).  The 16-row kernels write through (st_kx).
template <int H, int R, int CT>
__device__ __forceinline__ void h1_kx(unsigned short* __restrict__ H1x, unsigned short* __restrict__ dZ2x, int net,
                                      int mb, int r0, int n0, const unsigned (&h1w)[R / 16][CT][6]) {
  const int64_t PLX = kx_rows(mb) * H;                             // plane elements per net
  store_kx_w<H, R, CT, R == kRowsShort>(H1x + net * 3 * PLX, PLX, r0, n0, h1w);
  if (R < 32 && r0 + R < kx_rows(mb) && r0 + R >= mb) {            // (uniform) the padded chunk's rows past this block
    const float z[R / 16][CT][4] = {};
    store_kx<H, R, CT>(H1x + net * 3 * PLX, PLX, r0 + R, n0, z);
    store_kx<H, R, CT>(dZ2x + net * 3 * PLX, PLX, r0 + R, n0, z);
  }
}

// Shared-memory block and forward pass (phases A, B and the output-layer dot
// products of C) common to rowpass_kernel and policy_kernel, so the rollout's
// policy/value forward and the update's forward are the same instructions in
// the same order: logp_old from the rollout equals the update's first
// recomputation bit for bit, and every row's result is independent of N.
template <int H, int NW, int RR = kRows>
struct MlpSmem {
  static constexpr bool BF3 = kBf3<H>;
  static constexpr int R = RR, LDA = H + 4, LDS_S = 36;
  // bf16 planes: rows padded by 32 B, a row stride of 8 banks (mod 64): the
  // 16 lanes of each ds_read_b128 lane group ({0-3,12-15,20-27}, ...) of an
  // MFMA operand read (row i, 16-B column run g) then land on 16 distinct
  // 4-bank slots (8i + 4g mod 64).  A 16-B pad (4 banks) put two lanes of
  // every group on one slot: SQ_LDS_BANK_CONFLICT 1.67 M -> 0.49 M per
  // rowpass (tools/lds_conflict_ab.sh), bitwise the same, no faster
  static constexpr int LDP = H + 16, PS = R * LDP;
  float h1s[BF3 ? 0 : R][LDA] __attribute__((aligned(16)));                // tanh(fc1)
  unsigned short h1p[BF3 ? 3 * PS : 0] __attribute__((aligned(16)));      // (BF3) its three bf16 planes
  float S[R][LDS_S] __attribute__((aligned(16)));     // [s(18) | 1 | 0...] per row
  // per-column-tile output-layer partial sums, [row][output][tile] with the
  // tiles of a (row, output) contiguous (16-B aligned runs, padded to 4k+4
  // floats so the writers' rows 4 apart fall on different bank pairs): the
  // loss head reads each sum's partials as ds_read_b128s instead of one
  // ds_read per tile (the same partials, added in the same tile order)
  static constexpr int OSP = H / 16 + (H == 64 ? 8 : 4);
  float osum[R][3][OSP] __attribute__((aligned(16)));
};

// Rows r < nvalid of the block must be in S[r][0..17] when gather() returns;
// gather(tid, NT) runs while this wave's W1 rows are in flight.  On return
// acc = tanh(fc2) for this wave's columns, h1 = tanh(fc1) (for the fc1
// backward), w3 = this wave's output-layer weights, and osum holds the
// per-wave dot products (after a barrier).  h1out (nullable): row r of
// tanh(fc1) goes to h1out[r * H + n].  PRIO: the caller raised the wave's
// issue priority (s_setprio) for its weight loads; it drops back once phase
// B's are all out (the policy kernel, see there).  sync: how the phases wait
// for each other (RpBarrier / RpHandoff above; with RpHandoff osum is complete
// only after sync.wait_out(), which the caller issues where it reads osum).
// WMAG (the rowpass's D skip): the OR of the fc2.weight bits this wave loads
// in phase B goes into *wmag (RpFlags::wmag) before out is published.
template <int H, int NW, int R, bool APRE, bool PRIO = false, bool WMAG = false, class Gather,
          class Sync = RpBarrier>
__device__ __forceinline__ void mlp_forward(MlpSmem<H, NW, R>& sm, const float* __restrict__ P,
                                            int net, int nvalid,
                                            Gather gather, float* __restrict__ h1out,
                                            f4 (&acc)[R / 16][H / 16 / NW],
                                            float (&h1)[R / 16][H / 16 / NW][4],
                                            float (&w3)[H / 16 / NW][3],
                                            unsigned (&h1w)[R / 16][H / 16 / NW][6], Sync sync = Sync(),
                                            unsigned* wmag = nullptr) {
  static_assert(!WMAG || kBf3<H>, "the weight bits are collected in mfma_rows3");
  constexpr int RT = R / 16, LDA = H + 4, CT = H / 16 / NW, LDS_S = 36, NT = NW * 64;
  static_assert(CT >= 1 && H % (16 * NW) == 0, "tile split");
  static_assert(!Sync::kHandoff || kBf3<H>, "the hand-off form waits inside mfma_rows3");
  const Layout L = layout(H);
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, li = l & 15, lg = l >> 4;
  const int n0 = w * (H / NW);

  // ---- A: gather, fc1 on MFMA ------------------------------------------------
  // this wave's W1aug rows [n][20] (k 0..19, zero-padded to 32; lane group g
  // takes k = 8g .. 8g+7), issued first so they overlap the row gather.  The
  // loads are unconditional (in-row offsets clamped) and the zero padding is
  // selected only after the gather's barrier: a load inside a lane-group
  // branch made the wave wait for it before issuing its row loads
  // The fc2 bias and output-layer weights of this wave's columns (used in C)
  // go out with them: __syncthreads drains every outstanding load, so loads
  // issued after the gather would hold up the barrier below
  float4 w1raw[CT][2];
  float b2v[CT], w3raw[CT][3];
  {
    const float* W1 = P + L.W1 + (int64_t)net * H * 20;
    const int o0 = lg < 2 ? 8 * lg : 16, o1 = lg < 2 ? 8 * lg + 4 : 16;
#pragma unroll
    for (int t = 0; t < CT; ++t) {
      const int n = n0 + 16 * t + li;
      const float* bp = W1 + (int64_t)n * 20;
      w1raw[t][0] = *reinterpret_cast<const float4*>(bp + o0);
      w1raw[t][1] = *reinterpret_cast<const float4*>(bp + o1);
      b2v[t] = P[L.b2 + net * H + n];
      w3raw[t][0] = P[(net == 0 ? L.W3a : L.W3c) + n];
      w3raw[t][1] = P[L.W3a + H + n];
      w3raw[t][2] = P[L.W3a + 2 * H + n];
    }
  }
  gather(tid, NT);
  pad_rows<NT>(sm.S, nvalid);
  sync.init();
  PHASE_PROBE(8);
  rp_barrier();
  PHASE_PROBE(9);
  sync.after_gather();
  // (split-bf16 fc2) phase B's first weight chunks go out now, under fc1 (an
  // LDS-only barrier below, leaving them in flight, measured no faster)
  WPre<CT> preB;
  if constexpr (kBf3<H>) mfma_rows_pre<H, CT>(P + L.W2 + (int64_t)net * H * H, n0, preB);
  float4 bw1[CT][2];
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int t = 0; t < CT; ++t) {
    bw1[t][0] = lg < 3 ? w1raw[t][0] : z4;
    bw1[t][1] = lg < 2 ? w1raw[t][1] : z4;
    w3[t][0] = w3raw[t][0];                                       // actor: mean_layer rows, critic: fc3
    w3[t][1] = net == 0 ? w3raw[t][1] : 0.0f;
    w3[t][2] = net == 0 ? w3raw[t][2] : 0.0f;
  }
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int t = 0; t < CT; ++t) acc[rt][t] = f4{0.f, 0.f, 0.f, 0.f};
  mfma_chunk<LDS_S, RT, CT, 4>(&sm.S[li][8 * lg], bw1, acc);
  PHASE_PROBE(10);
  // fc1 + tanh: a column tile's RT * 4 values per call (tanh_f32_n, where kTanhArms)
  float hv[CT][RT * 4];
#pragma unroll
  for (int t = 0; t < CT; ++t) {
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int j = 0; j < 4; ++j) hv[t][4 * rt + j] = acc[rt][t][j];
    if constexpr (kTanhArms<H>) {
      tanh_f32_n(hv[t]);
    } else {
#pragma unroll
      for (int q = 0; q < RT * 4; ++q) hv[t][q] = tanh_f32(hv[t][q]);
    }
  }
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int t = 0; t < CT; ++t) {
      const int n = n0 + 16 * t + li;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = 16 * rt + 4 * lg + j;
        const float h = hv[t][4 * rt + j];
        h1[rt][t][j] = h;
        if constexpr (!kBf3<H>) sm.h1s[r][n] = h;
      }
      // (split-bf16) the three planes of the lane's four rows, split once as
      // pairs; the words stay in h1w for the k-packed H1 store (rowpass_kx)
      if constexpr (kBf3<H>)
        put3_col4<MlpSmem<H, NW, R>::PS, MlpSmem<H, NW, R>::LDP>(
            sm.h1p, (16 * rt + 4 * lg) * MlpSmem<H, NW, R>::LDP + n, h1[rt][t], h1w[rt][t]);
      acc[rt][t] = f4{0.f, 0.f, 0.f, 0.f};
    }
  if (h1out != nullptr) store_rows<R, CT>(h1out, H, n0, nvalid, h1);   // straight-line unless ragged
  PHASE_PROBE(11);
  sync.h1_written();                                               // (stamp 1 in there, or in B's first wait)

  // ---- B: Z2 = H1 W2^T -------------------------------------------------------
  unsigned wbits = 0u;
  if constexpr (kBf3<H>)
    mfma_rows3<H, MlpSmem<H, NW, R>::LDP, MlpSmem<H, NW, R>::PS, H, RT, CT, true, WMAG>(
        sm.h1p, P + L.W2 + (int64_t)net * H * H, n0, acc, &preB, sync.wait_h1(), &wbits);
  else
    mfma_rows<H, LDA, H, RT, CT, APRE>(&sm.h1s[0][0], P + L.W2 + (int64_t)net * H * H, n0, acc);
  if constexpr (PRIO) __builtin_amdgcn_s_setprio(0);
  PHASE_PROBE(2);

  // ---- C (forward part): fc2 tanh, output-layer dot products -----------------
  fc2_out_partials(acc, b2v, w3, net, li, lg, sm.osum, w * CT);
  if constexpr (WMAG) rp_or_put(wmag, wbits);
  sync.out_written();
  PHASE_PROBE(3);
}

// HANDOFF: the phases hand over by LDS words (RpHandoff) instead of workgroup
// barriers: the 32-row 16-wave k-packed kernel only, bitwise the same
template <int H, int NW, int R = kRows, bool FDW2 = false, bool KX = false, bool HANDOFF = false, bool SPAN = false>
__global__ void __launch_bounds__(NW * 64, NW * 64 / 256) rowpass_kernel(int mb, int net_sel,
                                                      const float* __restrict__ src, const int64_t* __restrict__ idx,
                                                      const float* __restrict__ P, const void* __restrict__ W2X,
                                                      float* __restrict__ H1g,
                                                      float* __restrict__ dZ2g, float epsilon, float ent_coef,
                                                      float max_action, float* __restrict__ ptail,
                                                      float* __restrict__ pw1, float* __restrict__ p2,
                                                      int S2, float* __restrict__ ratio_out, float inv_mb,
                                                      int dskip, unsigned long long* __restrict__ span) {
  // (argument order: the 14 dwords up to dZ2g are preloaded into SGPRs at wave
  // launch -- everything the block's net, the first weight loads and the row
  // gather need; the rest comes by s_load under them.  DESIGN.md 3.4.
  // dskip, the D skip's switch (satrl_ppo_rowpass_dskip), is the last argument
  // of the launch, before the span pointer launch_span appends.)
  const unsigned long long span_t0 = SPAN ? satrl_span::now() : 0ull;   // (SPAN: the measurement instantiation)
  constexpr int RT = R / 16, LDA = H + 4, CT = H / 16 / NW, NT = NW * 64;
  static_assert(!FDW2 || R == 32, "the fused dW2 partial covers one 32-row block (dw2_kernel's chunk)");
  // KX: H1 / dZ2 go out as k-packed bf16 planes (store_kx; H1g / dZ2g point at
  // u16 [2][3][kx_rows(mb)][H]) for satrl_ppo_dw2_kx, whole 32-row chunks (a
  // 16-row kernel's last block zero-fills the chunk's other half)
  static_assert(!KX || ((R == 32 || R == kRowsShort) && kBf3<H> && !FDW2), "k-packed outputs: split-bf16 width");
  static_assert(!HANDOFF || (KX && R == 32 && NW == 16), "hand-offs: the 32-row 16-wave k-packed kernel");
  const int64_t PLX = kx_rows(mb) * H;                             // (KX) plane elements per net
  const Layout L = layout(H);
  __shared__ MlpSmem<H, NW, R> sm;
  constexpr bool BF3 = kBf3<H>;
  constexpr int LDP = MlpSmem<H, NW, R>::LDP, PS = MlpSmem<H, NW, R>::PS;
  __shared__ __attribute__((aligned(16))) float dzs[BF3 ? 1 : R][BF3 ? 4 : LDA];   // dZ2
  __shared__ __attribute__((aligned(16))) unsigned short dzp[BF3 ? 3 * PS : 8];    // (BF3) its bf16 planes
  __shared__ float ax[R][8];
  __shared__ float dz3s[R][4];
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, li = l & 15, lg = l >> 4;
  // net_sel < 0: both nets, blockIdx = (row block, net); else that net only
  // XCD-matched placement (32-row k-packed kernel, both nets, a row-block
  // count divisible by 8): the row blocks of dW2 split s -- row blocks
  // [s nrb/8, (s+1) nrb/8), both nets -- go to the workgroups b with
  // b % 8 == s, i.e. under round-robin dispatch to the XCD that dw2_kx's
  // split s runs on (its block b takes split b % 8), so the planes dw2_kx
  // reads were written through that XCD's L2 (placement only: every bit is
  // the same; in-graph step at mb 4096 47.5-47.8 against 48.7-49.2 us over
  // three alternations, the rowpass->dw2 boundary 3.6-3.9 against 4.1-4.6
  // us; at mb 512 the 16-row kernel measured 0.2-0.3 us slower with it, so
  // it keeps the (row block, net) = (b / 2, b % 2) order; EXPERIMENTS.md
  // round 6).  Otherwise the actor lands on the even XCDs, the critic on the odd.
  const int nrbk = (mb + R - 1) / R;
  const bool xmap = KX && R == kRows && net_sel < 0 && nrbk % 8 == 0;
  const int bx = (int)blockIdx.x, kx8 = bx >> 3;
  const int net = net_sel < 0 ? (xmap ? (kx8 & 1) : (bx & 1)) : net_sel;
  const int rb = net_sel < 0 ? (xmap ? (bx & 7) * (nrbk >> 3) + (kx8 >> 1) : (bx >> 1)) : bx, n0 = w * (H / NW);
  const int r0 = rb * R;
  auto& S = sm.S;
#ifdef SATRL_PHASE_PROBE
  if (threadIdx.x == 0 && blockIdx.x < 512) {   // placement: XCC_ID and HW_ID (SE/SH/CU) of the workgroup
    g_probe[blockIdx.x][15][0][0] = __builtin_amdgcn_s_getreg((31 << 11) | 20);
    g_probe[blockIdx.x][15][0][1] = __builtin_amdgcn_s_getreg((31 << 11) | 4);
  }
#endif
  PHASE_PROBE(0);
  __shared__ float hcs[3][3];                                      // the head's constants (head_load)
  __shared__ float hb3s[4];
  float hls_d, hb3_d;
  head_load<H, NT>(P, hls_d, hb3_d);

  f4 acc[RT][CT];
  float h1[RT][CT][4];
  float w3[CT][3];
  unsigned h1w[RT][CT][6];                                         // (split-bf16) the split H1 words
  constexpr bool ESKIP = kZeroSkip<H, R>;                          // phase E's short cut, and its guard's words
  __shared__ unsigned nfw[ESKIP ? NW : 1];                         // per wave: gathered a non-finite state value
  auto gather = [&](int t0, int nt) {
    const bool fin = gather_rows<R, NT, !HANDOFF>(mb, src, idx, r0, t0, nt, S, ax, hls_d, hb3_d, hcs, hb3s);
    if constexpr (ESKIP) rows_finite_put(nfw, fin);
  };
  // how the phases wait for each other (RpBarrier / RpHandoff)
  __shared__ RpFlags flags;
  // the D skip (below, before phase D): the k-packed 32-row kernel, both sync forms
  constexpr bool DSKIP = kDSkip<H, R, KX>;
  auto sync = [&] {
    if constexpr (HANDOFF) return rp_handoff<NW>(flags, [&] { head_consts<NT>(hls_d, hb3_d, hcs, hb3s); });
    else if constexpr (DSKIP) return RpBarrierMag(flags);
    else return RpBarrier();
  }();
  // the fc2 operand image: the f32 W2^T
  const float* W2T = static_cast<const float*>(W2X);
  // (H = 256: the H1 store after phase B, not between fc1 and B: 8 fewer VGPRs
  // live through B, so the 32-row kernel stays at <= 104)
  // (FDW2, H = 64: at priority 3 until phase B's weight loads are out, as the
  // policy kernel -- in-graph step 18.2 against 18.4 us at configs[1]'s
  // mb 4096, 15.3 against 15.5 at 512; at H = 256 no gain, not set there)
  if constexpr (FDW2) __builtin_amdgcn_s_setprio(3);
    mlp_forward<H, NW, R, true, FDW2, DSKIP>(sm, P, net, mb - r0, gather,
                                          FDW2 || KX || BF3 ? nullptr : H1g + ((int64_t)net * mb + r0) * H, acc, h1,
                                          w3, h1w, sync, &flags.wmag);
  // (KX) the H1 planes: wave 0, which runs the loss head next, stores its
  // share after the head's barrier (hand-off), off the head's path; the
  // other waves now
  unsigned short* const H1x = reinterpret_cast<unsigned short*>(H1g);
  unsigned short* const dZ2x = reinterpret_cast<unsigned short*>(dZ2g);
  if constexpr (KX) {
    if (w != 0) h1_kx<H, R, CT>(H1x, dZ2x, net, mb, r0, n0, h1w);
  }
  else if constexpr (BF3 && !FDW2) store_rows<R, CT>(H1g + ((int64_t)net * mb + r0) * H, H, n0, mb - r0, h1);
  // ---- D skip (DSKIP; dskip: satrl_ppo_rowpass_dskip, 0 = phase D always runs) ----
  // dH1 has one use, phase E's dZ1 = dH1 (1 - H1^2).  A wave skips phase D and
  // phase E's MFMAs and stores +0.0 to its [dW1|db1] slab rows, the bytes the
  // full path gives, if
  //  (a) 1 - h^2 is +-0 for each of its own 32 x 16 H1 values (fc1 saturated:
  //      tanh_big returned +-1 exactly) -- one OR and one ballot, known here;
  //  (b) the block's gathered states are finite (nfw, phase E's guard: with a
  //      non-finite state E's MFMAs give NaNs that need the real dZ1);
  //  (c) dH1 is finite, shown without computing it.  With e_dz, e_w the biased
  //      exponent fields of RpFlags::dzmag / wmag (ORs of raw bits, so each is
  //      >= the field of every dZ2 value of the block / fc2.weight element of
  //      the net; 255 if any is inf or NaN): |x| < 2^(e - 126) for every such
  //      element, hence |s| <= 2^(e - 126) for each of its three bf16 splits
  //      (round to nearest never passes the next power of two).  An element of
  //      dH1 is the sum of at most 6 x 256 < 2^11 split products, each
  //      <= 2^(e_dz + e_w - 252), so every partial sum in the MFMA chain is
  //      <= 2^(11 + e_dz + e_w - 252), finite in f32 while e_dz + e_w <= 367.
  //      The test is e_dz != 255, e_w != 255, e_dz + e_w <= 360.
  //      (Phase D reads the W2X image where wmag saw P's fc2.weight: the image
  //      is that weight's transpose, include/satrl_ppo.h.)
  // Then dZ1 = finite x (+-0) = +-0 in every lane, and phase E's MFMAs add
  // +-0 x finite onto a +0 accumulator: +0.0 (phase_e's short cut, measured).
  // A wave for which (a) and (b) hold -- a candidate -- issues no early W2T
  // chunks, and after its tail waits for every wave's dZ2 (hand-off form: all
  // dz bits; barrier form: the barrier there is), reads the two words (wmag is
  // complete: the head ran behind every wave's out, the tail behind the head)
  // and, if (c) fails, issues the chunks then and runs D and E as every other
  // wave.  It writes its dZ2 planes, tail partials and plane stores first, as
  // every wave: others read them.  No wave waits for a skipping wave's D.
  bool cand = false;                                               // (wave-uniform)
  if constexpr (DSKIP) {
    unsigned nz = 0u;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int t = 0; t < CT; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) nz |= __float_as_uint(1.0f - h1[rt][t][j] * h1[rt][t][j]);
    cand = dskip != 0 && __builtin_amdgcn_ballot_w64((nz & 0x7fffffffu) != 0u) == 0 && rows_finite_all<NW>(nfw);
  }
  // phase D's first W2T chunks go out now, under the loss head and the tail
  WPre<CT> preD;
  if (!cand) mfma_rows_pre<H, CT>(W2T + (int64_t)net * H * H, n0, preD);

  // ---- C: the net's loss and its gradient, dZ2 ---------------------------------
  float* tp = ptail + (int64_t)rb * L.tail;                         // tail-relative slab of this row block
  sync.wait_out();                                                  // (hand-off: wave 0, for every wave's partials)
  loss_head<H, R, true>(mb, r0, net, inv_mb, epsilon, ent_coef, max_action, sm.osum, hcs, hb3s, ax, dz3s, tp,
                        ratio_out, true);
  sync.head_done();                                                 // dz3s is ready (stamp 4)
  // (wave 0's share of the H1 planes after the head's barrier: before it, the
  // barrier's vmcnt(0) waited for those stores' write latency with the other
  // 15 waves idle -- in-graph step 47.73-47.88 against 47.99-48.51 us over
  // four alternations, bitwise the same; EXPERIMENTS.md round 6)
  if constexpr (KX) {
    if (w == 0) h1_kx<H, R, CT>(H1x, dZ2x, net, mb, r0, n0, h1w);
  }
  float d2v[RT][CT][4];
  unsigned d2w[RT][CT][6];                                         // (split-bf16) the split dZ2 words
  tail<H, RT, CT, LDP, PS>(acc, w3, dz3s, &dzs[0][0], dzp, d2v, d2w, tp, net, n0);
  if constexpr (DSKIP) {                                               // (D skip) this wave's dZ2 bits, before dz
    unsigned dzb = 0u;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int t = 0; t < CT; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) dzb |= __float_as_uint(d2v[rt][t][j]);
    rp_or_put(&flags.dzmag, dzb);
  }
  if constexpr (HANDOFF) sync.dz_written();                            // (before the plane stores: they drain under D)
  if constexpr (KX)
    store_kx_w<H, R, CT, R == kRowsShort>(dZ2x + net * 3 * PLX, PLX, r0, n0, d2w);
  else if constexpr (!FDW2) store_rows<R, CT>(dZ2g + ((int64_t)net * mb + r0) * H, H, n0, mb - r0, d2v);
  if constexpr (!HANDOFF) sync.dz_written();                           // the barrier (stamp 5; hand-off: in D's first wait)

  float* const pw = pw1 + (int64_t)rb * 2 * H * 20 + (int64_t)net * H * 20;   // this net's [dW1|db1] slab
  bool skip = false;                                                   // (D skip) the candidate's decision, (c)
  if constexpr (DSKIP) {
    if (cand) {
      if constexpr (HANDOFF) {
        rp_wait(&flags.dz, (1u << NW) - 1u);                           // every wave's tail
        PHASE_PROBE(5);
      }
      const unsigned e_dz = (rp_read(&flags.dzmag) >> 23) & 0xffu, e_w = (rp_read(&flags.wmag) >> 23) & 0xffu;
      skip = e_dz != 255u && e_w != 255u && e_dz + e_w <= 360u;
      if (!skip) mfma_rows_pre<H, CT>(W2T + (int64_t)net * H * H, n0, preD);
    }
  }
  if (skip) {
    PHASE_PROBE(6);
    phase_e_zero<CT>(pw, n0);
    PHASE_PROBE(7);
  } else {
    // ---- D: dH1 = dZ2 W2 -----------------------------------------------------
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int t = 0; t < CT; ++t) acc[rt][t] = f4{0.f, 0.f, 0.f, 0.f};
    if constexpr (BF3)
      mfma_rows3<H, LDP, PS, H, RT, CT, true>(dzp, W2T + (int64_t)net * H * H, n0, acc, &preD, sync.wait_dz());
    else
      mfma_rows<H, LDA, H, RT, CT, true, true>(&dzs[0][0], W2T + (int64_t)net * H * H, n0, acc, &preD);
    PHASE_PROBE(6);

    // ---- E: dZ1 = dH1 (1 - H1^2); [dW1 | db1][n][k'] = sum_r dZ1[r][n] S[r][k'] ----
    phase_e<ESKIP, NW>(acc, h1, S, pw, n0, nfw);
    PHASE_PROBE(7);
  }

  // ---- F (FDW2, H <= 128): this block's dW2 partial = dZ2^T H1 over its rows ---
  // straight from the LDS images (dzs, h1s), written as split-K slab rb of
  // p2 [2][S2][H][H]: the MFMA sequence of dw2_kernel on one 32-row chunk
  // (A[n][k] = dZ2[row][n], B[k][m] = H1[row][m], row = 4ks + lg; rows past
  // the minibatch masked to 0), so the slab is bitwise dw2_kernel's with
  // S = the row-block count -- without the H1 / dZ2 round trip through HBM
  // and the dW2 launch.
  if constexpr (FDW2) {
    constexpr int MT = H / 16;
    const int nvalid = mb - r0;
#pragma unroll
    for (int t = 0; t < CT; ++t) {
      f4 a2[MT];
#pragma unroll
      for (int j = 0; j < MT; ++j) a2[j] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < R / 4; ++ks) {
        const int row = 4 * ks + lg;
        float a = dzs[row][n0 + 16 * t + li];
        if (row >= nvalid) a = 0.0f;
#pragma unroll
        for (int j = 0; j < MT; ++j) a2[j] = mfma4(a, sm.h1s[row][16 * j + li], a2[j]);
      }
      float* out = p2 + ((int64_t)net * S2 + rb) * H * H;
#pragma unroll
      for (int j = 0; j < MT; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          out[(int64_t)(n0 + 16 * t + 4 * lg + q) * H + 16 * j + li] = a2[j][q];
        }
    }
  }
  if constexpr (SPAN) satrl_span::exit(span, span_t0);
}

// ---------------------------------------------------------------------------
// rowpass_cs: the short-minibatch H = 256 k-packed rowpass (16-row blocks)
// with each (row block, net) split by hidden columns over kCsSplit workgroups
// of kCsWaves waves: quarter j owns the 16-column tiles 4j .. 4j+3, its wave w
// the tile 4j + w (columns 64j + 16w ..).  At configs[3]'s 512 rows per rank
// rowpass_kernel<256, 16, 16> puts 64 workgroups of 16 waves on 256 CUs, four
// waves per SIMD issuing phases B and D one after another; here 256
// workgroups of 4 waves, one wave per SIMD.  Every output is bitwise
// rowpass_kernel<256, 16, kRowsShort, false, true>'s: the head scalars, row
// gather, S padding, fc2 tanh and output-layer partials, loss head, tail,
// phase E and the H1 plane stores are that kernel's own functions (head_load
// .. h1_kx above) at RT = CT = 1, and phases B and D its mfma_rows3.  Written
// out here, because its shape differs: the fc1 prologue -- every quarter
// computes fc1 of all 16 tiles, four per wave (phase B's A operand is all of
// H1), in mlp_forward's per-tile sequence -- and with it the loads of the
// wave's fc2 bias and output-layer weights.
// Two hand-offs inside the launch between the kCsSplit workgroups of a group,
// in the form of row 3 of MI355X_MICROARCH.md's sc1 hand-off table: __device__
// arrays; payload stores sc1 (8 B, every 128-B line by 16 lanes of one store
// instruction); every storing wave's vmcnt(0) wait and a workgroup barrier
// before ONE agent-scope add per workgroup; a global_load_dword sc1 poll; a
// workgroup barrier between the poll and every payload load
// (buffer_load_dwordx4 sc1):
//   X1  each quarter's output-layer tile partials (the loss head sums all 16
//       tiles, in tile order, in every quarter);
//   X2  each quarter's columns of the dZ2 bf16 planes (phase D's k runs over
//       all 256).
// A group's counter only grows, by kCsSplit at each hand-off, so a launch
// finds it at 2 kCsSplit L (L = the group's launches so far) and the value
// an add returns names the launch's targets.  A wait longer than
// kCsTimeoutTicks (a group not co-resident: the launcher checks residency
// first) sets g_cs_err and leaves the kernel, so the grid always drains;
// satrl_ppo_rowpass_error reports it and re-arms the counters.
// ---------------------------------------------------------------------------
constexpr int kCsWaves = 4, kCsSplit = 256 / 16 / kCsWaves;   // waves per workgroup, workgroups per group
// minibatches of up to this many rows (the whole 16-row range: at mb 1024
// 512 workgroups, two per CU; in-graph step 33.2 against 35.5 us, at mb 768
// 32.2 against 34.4, three alternations; EXPERIMENTS.md round 6)
constexpr int kCsMaxMb = 1024;
constexpr int kCsMaxGroups = 2 * (kCsMaxMb / kRowsShort);      // (row block, net) groups
constexpr unsigned long long kCsTimeoutTicks = 50000000ull;     // 0.5 s of s_memrealtime (100 MHz)
__device__ __attribute__((aligned(128))) unsigned g_cs_ctr[kCsMaxGroups][32];   // a 128-B line per counter
__device__ __attribute__((aligned(128))) float g_cs_x1[kCsMaxGroups][kCsSplit][kRowsShort][3][kCsWaves];
__device__ __attribute__((aligned(128))) unsigned short g_cs_x2[kCsMaxGroups][3][kRowsShort][256];

// one hand-off step (1: X1, 2: X2) of a group: true once every workgroup of
// the group has published it, false (every thread) after a timeout
__device__ __forceinline__ bool cs_handoff(unsigned* ctr, unsigned step, unsigned* ok_lds) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");           // this wave's payload stores are out
  __syncthreads();                                            // ... and every other wave's
  if (threadIdx.x == 0) {
    const unsigned old = __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned target = old - old % (2u * kCsSplit) + step * kCsSplit;
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    unsigned ok = 1;
    while ((int)(__hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - target) < 0) {
      __builtin_amdgcn_s_sleep(1);
      if (__builtin_amdgcn_s_memrealtime() - t0 > kCsTimeoutTicks) {
        __hip_atomic_store(&g_cs_err[0], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ok = 0;
        break;
      }
    }
    *ok_lds = ok;
  }
  __syncthreads();
  return *ok_lds != 0;
}
// 16 B of a hand-off payload, from L2 (sc1: never a stale L1 line)
__device__ __forceinline__ float4 cs_load16(const void* base, int bytes, int off) {
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), (short)0, bytes, 0x00020000);
  return __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 16));
}
__device__ __forceinline__ void cs_store8(void* p, unsigned long long v) {
  __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <bool SPAN = false>
__global__ void __launch_bounds__(kCsWaves * 64) rowpass_cs_kernel(
    int mb, const float* __restrict__ src, const int64_t* __restrict__ idx, const float* __restrict__ P,
    const float* __restrict__ W2T, float epsilon, float ent_coef, float max_action,
    unsigned short* __restrict__ H1x, unsigned short* __restrict__ dZ2x, float* __restrict__ ptail,
    float* __restrict__ pw1, float inv_mb, unsigned long long* __restrict__ span) {
  const unsigned long long span_t0 = SPAN ? satrl_span::now() : 0ull;
  constexpr int H = 256, R = kRowsShort, NT = kCsWaves * 64, LDS_S = 36;
  constexpr int LDP = MlpSmem<H, 16, R>::LDP, PS = MlpSmem<H, 16, R>::PS, OSP = MlpSmem<H, 16, R>::OSP;
  struct Smem {
    unsigned short h1p[3 * PS];                  // tanh(fc1), all 256 columns, three bf16 planes
    unsigned short dzp[3 * PS];                  // dZ2 planes (this quarter's columns, then all)
    float S[R][LDS_S];
    float osum[R][3][OSP];                       // every tile's output-layer partials (after X1)
    float xs[R][3][kCsWaves];                    // this quarter's (X1 staging)
    float ax[R][8];
    float dz3s[R][4];
    float hcs[3][3];
    float hb3s[4];
    unsigned ok;
  };
  __shared__ __attribute__((aligned(16))) Smem sm;
  // group g = (row block, net), quarter j: blocks b, b + 8, b + 16, b + 24 of
  // each 32 form a group (one XCD under round-robin dealing: placement only)
  const int nrbk = (mb + R - 1) / R, ngrp = 2 * nrbk;
  const int bx = (int)blockIdx.x, j = (bx >> 3) & (kCsSplit - 1), grp = (bx & 7) | ((bx >> 5) << 3);
  if (grp >= ngrp) {                                               // (whole groups of the last window)
    if constexpr (SPAN) satrl_span::exit(span, span_t0);
    return;
  }
  const int net = grp & 1, rb = grp >> 1, r0 = rb * R;
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, li = l & 15, lg = l >> 4;
  const int n0 = 64 * j + 16 * w;                                  // this wave's tile: 4j + w
  const int64_t PLX = kx_rows(mb) * H;
  const Layout L = layout(H);
  unsigned* ctr = &g_cs_ctr[grp][0];
  PHASE_PROBE(0);

  float hls_d, hb3_d;
  head_load<H, NT>(P, hls_d, hb3_d);
  // fc1 weights of the wave's four fc1 tiles w, w + 4, w + 8, w + 12 (tile 4j + w
  // among them, t = j), this tile's fc2 bias and output-layer weights
  float4 w1raw[4][2];
  float b2v[1], w3raw[3];
  {
    const float* W1 = P + L.W1 + (int64_t)net * H * 20;
    const int o0 = lg < 2 ? 8 * lg : 16, o1 = lg < 2 ? 8 * lg + 4 : 16;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const float* bp = W1 + (int64_t)(16 * (w + 4 * t) + li) * 20;
      w1raw[t][0] = *reinterpret_cast<const float4*>(bp + o0);
      w1raw[t][1] = *reinterpret_cast<const float4*>(bp + o1);
    }
    const int n = n0 + li;
    b2v[0] = P[L.b2 + net * H + n];
    w3raw[0] = P[(net == 0 ? L.W3a : L.W3c) + n];
    w3raw[1] = P[L.W3a + H + n];
    w3raw[2] = P[L.W3a + 2 * H + n];
  }
  // ---- A: gather, fc1 of all 16 tiles ----------------------------------------
  gather_rows<R, NT>(mb, src, idx, r0, tid, NT, sm.S, sm.ax, hls_d, hb3_d, sm.hcs, sm.hb3s);
  pad_rows<NT>(sm.S, mb - r0);
  PHASE_PROBE(8);
  rp_barrier();
  PHASE_PROBE(9);
  WPre<1> preB;
  mfma_rows_pre<H, 1>(P + L.W2 + (int64_t)net * H * H, n0, preB);
  float w3[1][3];
  float4 bw1[4][2];
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    bw1[t][0] = lg < 3 ? w1raw[t][0] : z4;
    bw1[t][1] = lg < 2 ? w1raw[t][1] : z4;
  }
  w3[0][0] = w3raw[0];
  w3[0][1] = net == 0 ? w3raw[1] : 0.0f;
  w3[0][2] = net == 0 ? w3raw[2] : 0.0f;
  f4 a1[1][4];
#pragma unroll
  for (int t = 0; t < 4; ++t) a1[0][t] = f4{0.f, 0.f, 0.f, 0.f};
  mfma_chunk<LDS_S, 1, 4, 4>(&sm.S[li][8 * lg], bw1, a1);
  PHASE_PROBE(10);
  float h1[1][1][4];
  unsigned h1w[1][1][6];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    float hv[4];
    unsigned wd[6];
#pragma unroll
    for (int q = 0; q < 4; ++q) hv[q] = tanh_f32(a1[0][t][q]);
    put3_col4<PS, LDP>(sm.h1p, (4 * lg) * LDP + 16 * (w + 4 * t) + li, hv, wd);
    if (t == j) {
#pragma unroll
      for (int q = 0; q < 4; ++q) h1[0][0][q] = hv[q];
#pragma unroll
      for (int q = 0; q < 6; ++q) h1w[0][0][q] = wd[q];
    }
  }
  PHASE_PROBE(11);
  rp_barrier();
  PHASE_PROBE(1);
  // ---- B: this tile of Z2 = H1 W2^T ------------------------------------------
  f4 acc[1][1];
  acc[0][0] = f4{0.f, 0.f, 0.f, 0.f};
  mfma_rows3<H, LDP, PS, H, 1, 1, true>(sm.h1p, P + L.W2 + (int64_t)net * H * H, n0, acc, &preB);
  PHASE_PROBE(2);
  // the H1 k-packed planes of this tile (and the padded chunk's zero rows)
  h1_kx<H, R, 1>(H1x, dZ2x, net, mb, r0, n0, h1w);
  WPre<1> preD;
  mfma_rows_pre<H, 1>(W2T + (int64_t)net * H * H, n0, preD);
  // ---- C (forward): tanh(fc2), this tile's output-layer partials -> X1 -------
  fc2_out_partials(acc, b2v, w3, net, li, lg, sm.xs, w);
  PHASE_PROBE(3);
  rp_barrier();
  static_assert(sizeof(sm.xs) == 96 * 8, "X1 staging: 96 8-B stores, six 128-B lines");
  if (tid < 96)
    cs_store8(reinterpret_cast<unsigned long long*>(&g_cs_x1[grp][j][0][0][0]) + tid,
              reinterpret_cast<const unsigned long long*>(&sm.xs[0][0][0])[tid]);
  if (!cs_handoff(ctr, 1u, &sm.ok)) {
    if constexpr (SPAN) satrl_span::exit(span, span_t0);
    return;
  }
  PHASE_PROBE(12);
  if (tid < kCsSplit * R * 3) {                                    // every quarter's partials -> osum[r][q][4jq + w]
    const int jq = tid / (R * 3), rq = tid % (R * 3), r = rq / 3, q = rq % 3;
    *reinterpret_cast<float4*>(&sm.osum[r][q][4 * jq]) =
        cs_load16(&g_cs_x1[grp][0][0][0][0], (int)sizeof(g_cs_x1[0]), ((jq * R + r) * 3 + q) * 16);
  }
  rp_barrier();
  PHASE_PROBE(13);
  // ---- C: the loss head, in every quarter; quarter 0 stores ---------------------
  float* tp = ptail + (int64_t)rb * L.tail;
  loss_head<H, R, false>(mb, r0, net, inv_mb, epsilon, ent_coef, max_action, sm.osum, sm.hcs, sm.hb3s, sm.ax, sm.dz3s,
                         tp, nullptr, j == 0);
  rp_barrier();
  PHASE_PROBE(4);
  // ---- C: tail of this tile, dZ2 planes -> LDS, k-packed, X2 -------------------
  float d2v[1][1][4];
  unsigned d2w[1][1][6];
  tail<H, 1, 1, LDP, PS>(acc, w3, sm.dz3s, nullptr, sm.dzp, d2v, d2w, tp, net, n0);
  store_kx_w<H, R, 1, true>(dZ2x + net * 3 * PLX, PLX, r0, n0, d2w);
  rp_barrier();
  PHASE_PROBE(5);
  // this quarter's 64 columns of the three planes: 48 runs of 128 B, one run
  // per 16 lanes of one 8-B store instruction
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int u = tid + NT * k, c8 = u & 15, pr = u >> 4, p = pr / R, r = pr % R;
    cs_store8(&g_cs_x2[grp][p][r][64 * j + 4 * c8],
              *reinterpret_cast<const unsigned long long*>(&sm.dzp[p * PS + r * LDP + 64 * j + 4 * c8]));
  }
  if (!cs_handoff(ctr, 2u, &sm.ok)) {
    if constexpr (SPAN) satrl_span::exit(span, span_t0);
    return;
  }
  PHASE_PROBE(14);
  // the other quarters' columns -> dzp (16-B runs)
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const int u = tid + NT * k, c16 = u & 7, pr = (u >> 3) % (3 * R), jq = u / (8 * 3 * R);
    if (jq != j) {
      const int p = pr / R, r = pr % R, col = 64 * jq + 8 * c16;
      *reinterpret_cast<float4*>(&sm.dzp[p * PS + r * LDP + col]) =
          cs_load16(&g_cs_x2[grp][0][0][0], (int)sizeof(g_cs_x2[0]), ((p * R + r) * 256 + col) * 2);
    }
  }
  rp_barrier();
  // ---- D: this tile of dH1 = dZ2 W2 ------------------------------------------
  acc[0][0] = f4{0.f, 0.f, 0.f, 0.f};
  mfma_rows3<H, LDP, PS, H, 1, 1, true>(sm.dzp, W2T + (int64_t)net * H * H, n0, acc, &preD);
  PHASE_PROBE(6);
  // ---- E: dZ1, [dW1 | db1] rows of this tile ----------------------------------
  phase_e<false, kCsWaves>(acc, h1, sm.S, pw1 + (int64_t)rb * 2 * H * 20 + (int64_t)net * H * 20, n0, nullptr);
  PHASE_PROBE(7);
  if constexpr (SPAN) satrl_span::exit(span, span_t0);
}

// ---------------------------------------------------------------------------
// policy: the rollout's forward passes on the rowpass's own MLP code
// (mlp_forward), one workgroup per 32-row block and net.
//   MODE 0  actor -> mean = max_action*tanh(.) -> Normal sample -> clamp ->
//           per-dim log-prob (ppo_continuous.py:176-189) for `nagents`
//           parameter sets (blockIdx % nagents = agent: P0 pursuer, P1
//           evader; the actor is net 0 of each flat layout)
//   MODE 1  critic value (net 1 of P0), ppo_continuous.py:200-201
//   MODE 2  evaluation: MODE 0's forward and agent interleave, actions only.
//           Agent a with bit 1 << a of det_mask set acts with the mean,
//           max_action*tanh(.) (PPO_continuous.evaluate, ppo_continuous.py:
//           168-174); the other one with MODE 0's clamped sample, bit for bit
// ---------------------------------------------------------------------------
// rows per policy/value workgroup (64-row tiles measured 62 vs 58.5 us per
// rollout step at 16k envs: fewer, larger workgroups lose more to the tail
// than the halved weight ingest saves)
constexpr int kPolRows = 32;   // rows per policy workgroup
constexpr int kPolNW = 8;      // waves per policy workgroup at H = 256 (16: 61.6 vs 52.3 us per rollout step;
                               // with the wave priority 46.5-47.6 vs 45.1-45.2 us per launch)

// The body of both __global__ forms below.  POOL (MODE 0, two agents): agent
// `pool_agent`'s workgroups take their parameter base from a stored snapshot,
//   m = member[block];  P = 0 <= m < K ? pool + m * pool_stride : the live P0 / P1
// (block = blockIdx.x / nagents; one unsigned compare, so no device value of m
// addresses anything outside pool).  member[block] is one more dependent load
// ahead of the weight stream: it is issued first, and a full block's
// observation float4, which does not depend on it, goes out under it rather
// than behind the W1 rows that do.  With POOL false every pool argument is
// dead and the code is policy_kernel's as it was (the
// resource tables).  LEAGUE (the pooled form with a law table, DESIGN.md
// 3.2.3): K <= m < K + J names law m - K, and that workgroup branches
// uniformly round the whole MLP -- no parameter, no LDS access, no barrier --
// its lanes r < nvalid evaluating the law on obs_law and writing +0.0f
// log-probs.  j is formed from the first lane's m (readfirstlane): law_row
// reads the law through the constant address space, which needs a provably
// wave-uniform address.  With LEAGUE false obs_law, laws and J are dead and the
// instantiations are as they were (3.2.3, the resource tables).
template <int H, int NW, int MODE, bool SPAN, bool POOL, bool LEAGUE = false>
__device__ __forceinline__ void policy_body(int64_t N, const float* __restrict__ obs, const float* __restrict__ P0,
                                            const float* __restrict__ P1, int nagents, float max_action, uint32_t k00,
                                            uint32_t k01, uint32_t k10, uint32_t k11, int64_t env_offset,
                                            uint64_t step, const uint64_t* __restrict__ step_base,
                                            float* __restrict__ act0, float* __restrict__ logp0,
                                            float* __restrict__ act1, float* __restrict__ logp1,
                                            float* __restrict__ value, int det_mask,
                                            unsigned long long* __restrict__ span, const float* __restrict__ pool,
                                            const int32_t* __restrict__ member, int64_t pool_stride, int K,
                                            int pool_agent, const float* __restrict__ obs_law = nullptr,
                                            const satrl_scripted_law* __restrict__ laws = nullptr, int J = 0) {
  static_assert(!POOL || (MODE == 0 && !SPAN), "the pooled form is the product MODE 0 kernel");
  static_assert(!LEAGUE || POOL, "the league form is the pooled one with a law table");
  const unsigned long long span_t0 = SPAN ? satrl_span::now() : 0ull;
  constexpr int R = kPolRows, RT = R / 16, CT = H / 16 / NW;
  // Two or more workgroups share a CU, and one finishing its output layer
  // would out-issue (oldest first) one that is still streaming W1 / W2: at
  // priority 3 until phase B's weight loads are out, a starting workgroup's
  // loads go first and overlap the other's tail (46 against 49 us per H 256
  // launch at 16 384 envs; bitwise unchanged)
  __builtin_amdgcn_s_setprio(3);
  const Layout L = layout(H);
  __shared__ MlpSmem<H, NW, R> sm;
  const int agent = MODE != 1 ? (int)(blockIdx.x % nagents) : 0;
  const int64_t r0 = (int64_t)(MODE != 1 ? blockIdx.x / nagents : blockIdx.x) * R;
  int m = -1;
  if constexpr (POOL)
    if (agent == pool_agent) m = member[blockIdx.x / nagents];   // (uniform branch: the other agent's workgroups load nothing more)
  const float* P = agent == 0 ? P0 : P1;
  const int nvalid = (int)(N - r0 < R ? N - r0 : R);
  float4 pre = make_float4(0.f, 0.f, 0.f, 0.f);                   // (POOL) a full block's float4, in flight under member[block]
  if constexpr (POOL) {
    const float* ob = obs + r0 * 18;
    if (nvalid == R && (reinterpret_cast<uintptr_t>(ob) & 15) == 0 && (int)threadIdx.x < R * 18 / 4)
      pre = reinterpret_cast<const float4*>(ob)[threadIdx.x];
    if ((unsigned)m < (unsigned)K) P = pool + (int64_t)m * pool_stride;   // (m stays -1 for the other agent; K > 0)
  }
  if constexpr (LEAGUE) {
    // m - K in unsigned arithmetic: every m outside [K, K + J) wraps past J (J <= 8), the other agent's -1 too
    const unsigned j = (unsigned)__builtin_amdgcn_readfirstlane(m) - (unsigned)K;
    if (j < (unsigned)J) {                                       // (uniform: the whole workgroup leaves here)
      const int r = threadIdx.x;
      if (r < nvalid) {
        const int64_t i = r0 + r;
        satrl_scripted::law_row(laws + j, obs_law + i * 18, (agent == 0 ? act0 : act1) + i * 3);
        float* lp = (agent == 0 ? logp0 : logp1) + i * 3;
        lp[0] = 0.0f;
        lp[1] = 0.0f;
        lp[2] = 0.0f;
      }
      return;
    }
  }
  auto gather = [&](int t0, int nt) {
    const float* ob = obs + r0 * 18;
    if (nvalid == R && (reinterpret_cast<uintptr_t>(ob) & 15) == 0) {
      // a full block's R x 18 floats are one contiguous 16-B-aligned span:
      // every float4 in flight at once (R * 18 / 4 <= one per thread)
      static_assert(R * 18 / 4 <= 4 * 64, "one float4 per thread of the smallest workgroup");
      if (t0 < R * 18 / 4) {
        const float4 v = POOL ? pre : reinterpret_cast<const float4*>(ob)[t0];
        const float e4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int q = 4 * t0 + e;
          sm.S[q / 18][q % 18] = e4[e];
        }
      }
    } else {
      for (int q = t0; q < R * 18; q += nt) {
        const int r = q / 18, c = q % 18;
        sm.S[r][c] = r < nvalid ? obs[(r0 + r) * 18 + c] : 0.0f;
      }
    }
  };
  f4 acc[RT][CT];
  float h1[RT][CT][4];
  float w3[CT][3];
  unsigned h1w[RT][CT][6];
  mlp_forward<H, NW, R, false, true>(sm, P, MODE != 1 ? 0 : 1, nvalid, gather, nullptr, acc, h1, w3, h1w);
  const int r = threadIdx.x;
  if (r >= nvalid) {                                             // no barrier follows
    if constexpr (SPAN) satrl_span::exit(span, span_t0);
    return;
  }
  const int64_t i = r0 + r;
  if (MODE == 1) {
    value[i] = out_sum<H / 16>(sm.osum, r, 0) + P[L.b3c];
    if constexpr (SPAN) satrl_span::exit(span, span_t0);
    return;
  }
  float* act = agent == 0 ? act0 : act1;
  if constexpr (MODE == 2) {
    if ((det_mask >> agent) & 1) {                               // (uniform: the workgroup's agent)
#pragma unroll
      for (int d = 0; d < 3; ++d)
        act[i * 3 + d] = max_action * tanh_f32(out_sum<H / 16>(sm.osum, r, d) + P[L.b3a + d]);   // evaluate()
      if constexpr (SPAN) satrl_span::exit(span, span_t0);
      return;
    }
  }
  float z[4];
  philox_normal4((uint64_t)(env_offset + i), step + (step_base ? *step_base : 0ull), agent == 0 ? k00 : k10,
                 agent == 0 ? k01 : k11, z);
  if constexpr (MODE == 2) {
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const float mu = max_action * tanh_f32(out_sum<H / 16>(sm.osum, r, d) + P[L.b3a + d]);
      float lp;                                                  // (dead: MODE 0's expression for the action alone)
      gaussian_act(mu, P[L.ls + d], z[d], max_action, act[i * 3 + d], lp);
    }
    if constexpr (SPAN) satrl_span::exit(span, span_t0);
    return;
  }
  float* logp = agent == 0 ? logp0 : logp1;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const float mu = max_action * tanh_f32(out_sum<H / 16>(sm.osum, r, d) + P[L.b3a + d]);   // 1.6 * tanh(mean_layer)
    gaussian_act(mu, P[L.ls + d], z[d], max_action, act[i * 3 + d], logp[i * 3 + d]);
  }
  if constexpr (SPAN) satrl_span::exit(span, span_t0);
}

template <int H, int NW, int MODE, bool SPAN = false>
__global__ void __launch_bounds__(NW * 64) policy_kernel(int64_t N, const float* __restrict__ obs,
                                                     const float* __restrict__ P0, const float* __restrict__ P1,
                                                     int nagents, float max_action, uint32_t k00, uint32_t k01,
                                                     uint32_t k10, uint32_t k11, int64_t env_offset, uint64_t step,
                                                     const uint64_t* __restrict__ step_base,
                                                     float* __restrict__ act0, float* __restrict__ logp0,
                                                     float* __restrict__ act1, float* __restrict__ logp1,
                                                     float* __restrict__ value, int det_mask,
                                                     unsigned long long* __restrict__ span) {
  policy_body<H, NW, MODE, SPAN, false>(N, obs, P0, P1, nagents, max_action, k00, k01, k10, k11, env_offset, step,
                                        step_base, act0, logp0, act1, logp1, value, det_mask, span, nullptr, nullptr,
                                        0, 0, 0);
}

// The pooled MODE 0 kernel (satrl_policy_act_pool), both agents.  Its first
// 14 argument dwords (kernarg preload) are what its first loads
// need: N, obs, pool, member, pool_stride, K, pool_agent, P0 (P1 follows by
// s_load; packing the stride and K so that it fits too measured no faster,
// EXPERIMENTS.md).  There is no SPAN instantiation: while a span probe is set
// a pooled launch runs this kernel and logs nothing.
template <int H, int NW>
__global__ void __launch_bounds__(NW * 64) policy_pool_kernel(int64_t N, const float* __restrict__ obs,
                                                          const float* __restrict__ pool,
                                                          const int32_t* __restrict__ member, int64_t pool_stride,
                                                          int K, int pool_agent, const float* __restrict__ P0,
                                                          const float* __restrict__ P1, float max_action, uint32_t k00,
                                                          uint32_t k01, uint32_t k10, uint32_t k11,
                                                          int64_t env_offset, uint64_t step,
                                                          const uint64_t* __restrict__ step_base,
                                                          float* __restrict__ act0, float* __restrict__ logp0,
                                                          float* __restrict__ act1, float* __restrict__ logp1) {
  policy_body<H, NW, 0, false, true>(N, obs, P0, P1, 2, max_action, k00, k01, k10, k11, env_offset, step, step_base,
                                     act0, logp0, act1, logp1, nullptr, 0, nullptr, pool, member, pool_stride, K,
                                     pool_agent);
}

// The league MODE 0 kernel (satrl_policy_act_league): the pooled kernel with a
// table of J laws behind the K stored sets.  Its first 14 argument dwords are
// what either branch's first loads and the branch itself need: N, obs, pool,
// member, pool_stride, K, pool_agent, J and max_action (P0, P1, obs_law and
// laws follow by s_load under the member load).  No SPAN instantiation, as
// for the pooled kernel.
template <int H, int NW>
__global__ void __launch_bounds__(NW * 64) policy_league_kernel(int64_t N, const float* __restrict__ obs,
                                                            const float* __restrict__ pool,
                                                            const int32_t* __restrict__ member, int64_t pool_stride,
                                                            int K, int pool_agent, int J, float max_action,
                                                            const float* __restrict__ P0,
                                                            const float* __restrict__ P1,
                                                            const float* __restrict__ obs_law,
                                                            const satrl_scripted_law* __restrict__ laws, uint32_t k00,
                                                            uint32_t k01, uint32_t k10, uint32_t k11,
                                                            int64_t env_offset, uint64_t step,
                                                            const uint64_t* __restrict__ step_base,
                                                            float* __restrict__ act0, float* __restrict__ logp0,
                                                            float* __restrict__ act1, float* __restrict__ logp1) {
  policy_body<H, NW, 0, false, true, true>(N, obs, P0, P1, 2, max_action, k00, k01, k10, k11, env_offset, step,
                                           step_base, act0, logp0, act1, logp1, nullptr, 0, nullptr, pool, member,
                                           pool_stride, K, pool_agent, obs_law, laws, J);
}

// ---------------------------------------------------------------------------
// Scripted opponents: one agent of the rollout acts with a
// linear guidance law (scripted_device.h) instead of a network.
//   scripted_kernel          the law alone, a lane per env row
//   policy_scripted_kernel   the learner's MODE 0 / MODE 2 forward in
//                            policy_kernel's one-agent grid (workgroups
//                            0 .. nblk-1, policy_body as policy_kernel
//                            instantiates it) and, behind them, a tail of
//                            workgroups that branch uniformly round the MLP
//                            and evaluate the law, a lane per row: no
//                            parameter, no LDS, no log-prob.
// The learner's Philox key arrives as (k0, k1): the host passes the key
// stream of the learner's agent id, so an evader learner draws agent 1's
// noise although its workgroups run as policy_body's agent 0.  The first 14
// argument dwords (kernarg preload) are N, obs, P, obs_law, law, act_scripted,
// nblk and max_action: what either branch's first loads need.
// ---------------------------------------------------------------------------
constexpr int kScriptedBlock = 256;   // rows per workgroup of scripted_kernel

__global__ void __launch_bounds__(kScriptedBlock) scripted_kernel(int64_t N, const float* __restrict__ obs,
                                                                  const satrl_scripted_law* __restrict__ law,
                                                                  float* __restrict__ act) {
  const int64_t i = (int64_t)blockIdx.x * kScriptedBlock + threadIdx.x;
  if (i < N) satrl_scripted::law_row(law, obs + i * 18, act + i * 3);
}

template <int H, int NW, int MODE>
__global__ void __launch_bounds__(NW * 64) policy_scripted_kernel(int64_t N, const float* __restrict__ obs,
                                                              const float* __restrict__ P,
                                                              const float* __restrict__ obs_law,
                                                              const satrl_scripted_law* __restrict__ law,
                                                              float* __restrict__ act_scripted, int nblk,
                                                              float max_action, uint32_t k0, uint32_t k1,
                                                              int64_t env_offset, uint64_t step,
                                                              const uint64_t* __restrict__ step_base,
                                                              float* __restrict__ act, float* __restrict__ logp,
                                                              int det) {
  static_assert(MODE == 0 || MODE == 2, "the act and the eval form");
  if ((int)blockIdx.x >= nblk) {                                  // (uniform: the scripted agent's workgroups)
    const int64_t i = (int64_t)((int)blockIdx.x - nblk) * (NW * 64) + threadIdx.x;
    if (i < N) satrl_scripted::law_row(law, obs_law + i * 18, act_scripted + i * 3);
    return;
  }
  policy_body<H, NW, MODE, false, false>(N, obs, P, nullptr, 1, max_action, k0, k1, 0u, 0u, env_offset, step,
                                         step_base, act, logp, nullptr, nullptr, nullptr, det, nullptr, nullptr,
                                         nullptr, 0, 0, 0);
}

// ---------------------------------------------------------------------------
// Update diagnostics (satrl_ppo_diagnostics): the forward pass of both nets
// over rows src[idx[r]] of the packed table and, per (32-row block, net)
// workgroup, f64 partial sums of what the loss head sees -- the policy
// kernel's shape (kPolRows rows, its wave counts and its wave priority) on the
// rowpass's gather, head constants and mlp_forward, so ratio and v are the
// update's own bits.  No gradient, nothing of the update is written.
// A block's partial is one 128-B line of `part` f64 [row block][16]:
//   actor  [0..7]  rows, sum min(s1, s2), sum kl, sum d, clipped rows, max ratio, 0, 0
//   critic [8..15] sum (v - vt)^2, sum (vt - v), sum vt, sum vt^2, 0, 0, 0, 0
// Lanes 0..31 of wave 0 hold a row each; lane q < 8 then adds the block's 32
// values of slot q in row order (rows past n contribute 0), so a partial
// depends on the block's rows alone.  diag_reduce_kernel adds the lines.
// ---------------------------------------------------------------------------
constexpr int kDiagLine = 16;       // f64 per row block of `part`
constexpr int kDiagChunk = 4096;    // lines per workgroup of the first reduce level

template <int H, int NW>
__global__ void __launch_bounds__(NW * 64) diag_kernel(int n, const float* __restrict__ src,
                                                       const int64_t* __restrict__ idx, const float* __restrict__ P,
                                                       float epsilon, float max_action, double* __restrict__ part,
                                                       float* __restrict__ rows_out) {
  constexpr int R = kPolRows, RT = R / 16, CT = H / 16 / NW, NT = NW * 64;
  __builtin_amdgcn_s_setprio(3);                                  // (as policy_kernel: until phase B's loads are out)
  __shared__ MlpSmem<H, NW, R> sm;
  __shared__ float ax[R][8];
  __shared__ float hcs[3][3];
  __shared__ float hb3s[4];
  __shared__ double red[5][R + 1];                                 // (+1: the adding lanes on distinct banks)
  const int net = (int)blockIdx.x & 1, rb = (int)blockIdx.x >> 1, r0 = rb * R;
  float hls_d, hb3_d;
  head_load<H, NT>(P, hls_d, hb3_d);
  f4 acc[RT][CT];
  float h1[RT][CT][4];
  float w3[CT][3];
  unsigned h1w[RT][CT][6];
  auto gather = [&](int t0, int nt) {
    gather_rows<R, NT>(n, src, idx, r0, t0, nt, sm.S, ax, hls_d, hb3_d, hcs, hb3s);
  };
  mlp_forward<H, NW, R, false, true>(sm, P, net, n - r0, gather, nullptr, acc, h1, w3, h1w);
  const int r = threadIdx.x, row = r0 + r;
  if (r < R) {
    double q[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (row < n) {
      if (net == 0) {
        // (the loss head's f32 expressions, in its order)
        float logp[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          const float th = tanh_f32(out_sum<H / 16>(sm.osum, r, d) + hb3s[d]);
          const float mu = max_action * th;
          const float var = hcs[0][d];
          const float dv = ax[r][d] - mu;
          logp[d] = (-(dv * dv) / (2.0f * var) - hcs[1][d]) - kLogSqrt2Pi;
        }
        const float lsum = (logp[0] + logp[1]) + logp[2];
        const float lold = (ax[r][3] + ax[r][4]) + ax[r][5];
        const float dl = lsum - lold;
        const float ratio = expf(dl);
        const float adv = ax[r][6];
        const float s1 = ratio * adv;
        const float cr = fminf(fmaxf(ratio, 1.0f - epsilon), 1.0f + epsilon);
        const float s2 = cr * adv;
        const bool clipped = ratio < 1.0f - epsilon || ratio > 1.0f + epsilon;
        q[0] = fmin((double)s1, (double)s2);
        q[1] = ((double)ratio - 1.0) - (double)dl;
        q[2] = (double)dl;
        q[3] = clipped ? 1.0 : 0.0;
        q[4] = (double)ratio;
        if (rows_out != nullptr) {
          rows_out[(int64_t)row * 4 + 0] = ratio;
          rows_out[(int64_t)row * 4 + 1] = dl;
        }
      } else {
        const float vc = out_sum<H / 16>(sm.osum, r, 0) + hb3s[3];
        const double vt = (double)ax[r][7], e = (double)vc - vt;
        q[0] = e * e;
        q[1] = -e;
        q[2] = vt;
        q[3] = vt * vt;
        if (rows_out != nullptr) {
          rows_out[(int64_t)row * 4 + 2] = vc;
          rows_out[(int64_t)row * 4 + 3] = 0.0f;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) red[k][r] = q[k];
  }
  __syncthreads();
  if (r < 8) {
    // actor: slot 0 the row count, 1..4 sums of red[0..3], 5 the max of red[4];
    // critic: slots 0..3 sums of red[0..3]
    const int k = net == 0 ? r - 1 : r;
    double s = 0.0;
    if (k >= 0 && k < 4) {
      for (int i = 0; i < R; ++i) s += red[k][i];
    } else if (net == 0 && r == 5) {
      for (int i = 0; i < R; ++i) s = fmax(s, red[4][i]);
    } else if (net == 0 && r == 0) {
      s = (double)(n - r0 < R ? n - r0 : R);
    }
    part[(int64_t)rb * kDiagLine + 8 * net + r] = s;
  }
}

// out line b = the lines in[b * chunk .. (b + 1) * chunk) added in a fixed
// order (slot 5: their max): thread (j, slot) of the 64 x 16 takes lines j,
// j + 64, ... of the chunk in turn, then slot threads of j = 0 add the 64
// partials in j order.  `final`: the one workgroup writes the SATRL_DIAG_N
// slots of `sums` instead of a line.
__global__ void __launch_bounds__(1024) diag_reduce_kernel(const double* __restrict__ in, int64_t nin, int chunk,
                                                           double* __restrict__ out, int final) {
  __shared__ double sh[64][kDiagLine + 1];
  const int t = threadIdx.x, slot = t & 15, j = t >> 4;
  const int64_t b0 = (int64_t)blockIdx.x * chunk;
  const int64_t b1 = b0 + chunk < nin ? b0 + chunk : nin;
  double s = 0.0;
  if (slot == 5) {
    for (int64_t b = b0 + j; b < b1; b += 64) s = fmax(s, in[b * kDiagLine + slot]);
  } else {
    for (int64_t b = b0 + j; b < b1; b += 64) s += in[b * kDiagLine + slot];
  }
  sh[j][slot] = s;
  __syncthreads();
  if (j != 0) return;
  s = sh[0][slot];
  for (int k = 1; k < 64; ++k) s = slot == 5 ? fmax(s, sh[k][slot]) : s + sh[k][slot];
  if (!final) {
    out[(int64_t)blockIdx.x * kDiagLine + slot] = s;
  } else if (slot < 6) {
    out[slot] = s;                                                 // rows .. ratio max
  } else if (slot >= 8 && slot < 12) {
    out[slot - 2] = s;                                             // value error^2 .. vt^2
  }
}

// ---------------------------------------------------------------------------
// dW2 = dZ2^T H1 per net (fc2.weight.grad), split-K over the minibatch rows.
// Workgroup (net, 64x64 output tile, split s) sums rows [s*KR, (s+1)*KR) of
// its tile into slab p2[net][s] with f32 MFMA 16x16x4 (4 waves; wave w owns
// tile rows 16w.., all four 16-column tiles).  32-row chunks of dZ2 and H1
// stream global -> LDS by LDS-DMA (global_load_lds_dwordx4) through a ring of
// kDwD slots with kDwD-1 chunks in flight: counted vmcnt + raw s_barrier, no
// VGPR staging.  The LDS image is XOR-swizzled on the source address (16-float
// groups ^ row&3) so the MFMA operand reads are bank-conflict free.  Block
// b -> split b % S: with S = 8 every split's 16 tiles share one XCD's L2.
// Every sum has a fixed order.
// ---------------------------------------------------------------------------
constexpr int kDwKC = 32, kDwD = 4;   // rows per chunk, ring slots (4/6/8 slots measured alike)
typedef __attribute__((address_space(3))) void lds_void_t;

template <int H>
__global__ void __launch_bounds__(256) dw2_kernel(int mb, int S, int KR, int net_sel, const float* __restrict__ H1g,
                                                  const float* __restrict__ dZ2g, float* __restrict__ p2) {
  constexpr int TT = H / 64;
  __shared__ __attribute__((aligned(16))) float ring[kDwD][2][kDwKC][64];   // [slot][dZ2 | H1][row][64 cols]
  const int t = threadIdx.x, w = t >> 6, l = t & 63, li = l & 15, lg = l >> 4;
  const int b = blockIdx.x, s = b % S, tile = (b / S) % (TT * TT);
  const int net = net_sel < 0 ? b / (S * TT * TT) : net_sel;
  const int n0 = (tile / TT) * 64, m0 = (tile % TT) * 64;
  const int r_begin = s * KR, nvalid = min(mb, r_begin + KR) - r_begin;
  const float* Z = dZ2g + (int64_t)net * mb * H;
  const float* Y = H1g + (int64_t)net * mb * H;
  const int nchunks = KR / kDwKC;
  // wave w stages rows 8w..8w+7 of a chunk: two 1-KB pieces (4 rows x 64 floats) per operand
  auto stage = [&](int c) {
    const int slot = c % kDwD;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int row = 8 * w + 4 * u + (l >> 4), c4 = (l & 15) ^ (4 * (row & 3));   // swizzled source
      const int r = min(r_begin + c * kDwKC + row, mb - 1);                       // rows past the end: masked below
      __builtin_amdgcn_global_load_lds(Z + (int64_t)r * H + n0 + 4 * c4, (lds_void_t*)&ring[slot][0][8 * w + 4 * u][0],
                                       16, 0, 0);
      __builtin_amdgcn_global_load_lds(Y + (int64_t)r * H + m0 + 4 * c4, (lds_void_t*)&ring[slot][1][8 * w + 4 * u][0],
                                       16, 0, 0);
    }
  };
  f4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int c = 0; c < kDwD - 1; ++c) stage(c < nchunks ? c : nchunks - 1);
  for (int c = 0; c < nchunks; ++c) {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"((kDwD - 2) * 4) : "memory");   // this wave's part of chunk c landed
    __builtin_amdgcn_s_barrier();                                            // every wave's part; slot c-1 free
    stage(c + kDwD - 1 < nchunks ? c + kDwD - 1 : nchunks - 1);             // (tail: a harmless reload)
    const int slot = c % kDwD, rows = nvalid - c * kDwKC;                    // rows >= `rows` are not ours
    // all of the chunk's operands first (40 ds_reads in flight), then the MFMAs
    float a[kDwKC / 4], bm[kDwKC / 4][4];
#pragma unroll
    for (int ks = 0; ks < kDwKC / 4; ++ks) {
      // A[n][k] = dZ2[row][n 16w+li], B[k][m] = H1[row][m 16j+li], row = 4ks+lg (row & 3 == lg)
      const int row = 4 * ks + lg;
      a[ks] = ring[slot][0][row][16 * (w ^ lg) + li];
      if (row >= rows) a[ks] = 0.0f;
#pragma unroll
      for (int j = 0; j < 4; ++j) bm[ks][j] = ring[slot][1][row][16 * (j ^ lg) + li];
    }
#pragma unroll
    for (int ks = 0; ks < kDwKC / 4; ++ks)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = mfma4(a[ks], bm[ks][j], acc[j]);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  // acc[j][q] = dW2[n0 + 16w + 4lg + q][m0 + 16j + li]
  float* out = p2 + ((int64_t)net * S + s) * H * H;
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int q = 0; q < 4; ++q) out[(int64_t)(n0 + 16 * w + 4 * lg + q) * H + m0 + 16 * j + li] = acc[j][q];
}

// ---------------------------------------------------------------------------
// dW2 at H = 256 from k-packed bf16 planes (satrl_ppo_dw2_kx): the rowpass
// wrote H1 and dZ2 already split and laid out so that the reduction index
// (rows) runs along each 16-B run (store_kx), so no transpose, no split and
// no VGPR staging is left here.  Workgroup (net, 64x64 output tile, split s)
// sums rows [s*KR, (s+1)*KR) into slab p2[net][s]; its 4 waves own 32x32
// quarters (2 x 2 v_mfma_f32_16x16x32_bf16 tiles, six partial products
// each, smallest first, as the rowpass).  Each 32-row chunk of the tile's
// operands -- 2 tensors x 3 planes x 4 row groups x 64 columns x 16 B = 24 KB
// -- streams global -> LDS by LDS-DMA (global_load_lds_dwordx4, one 1-KB run
// per instruction, six per wave) through a kKxD-slot ring with counted vmcnt
// and raw s_barrier; the MFMA operands are ds_read_b128 of consecutive 16-B
// (row groups 16 B apart in bank space).  Every sum has a fixed order.
//
// Each wave runs the chunk loop as a software pipeline: chunk c's 24 MFMAs
// issue from one operand register set while chunk c+1's 12 ds_read_b128 fill
// the other (in pairs, in first-use order) and the wave's six pieces of chunk
// c+kKxAhead go out between them, one piece or one read pair per MFMA gap
// over the chunk's first twelve MFMAs.  One s_barrier per chunk: behind it
// every wave's pieces of chunk c+1 have landed and every wave's reads of the
// slot about to be restaged are done.
// ---------------------------------------------------------------------------
constexpr int kKxD = 3;        // ring slots (four: one workgroup per CU, the fused launch's reduce blocks wait: slower)
// chunks the stream runs ahead of the MFMAs: kKxD (the slot restaged in
// iteration c is chunk c's, already in registers; its reads are waited for in
// front of the barrier) or kKxD - 1 (chunk c-1's; no LDS wait at the barrier)
constexpr int kKxAhead = 3;
static_assert(kKxAhead >= 2 && (kKxAhead == kKxD || kKxAhead == kKxD - 1), "see dw2_kx_body's barrier");
// where a chunk's LDS reads (in pairs) and LDS-DMA pieces sit among its 24 MFMAs: pieces behind MFMAs 0, 2, .. 10,
// read pairs behind 1, 3, .. 11 (dW2 span 8.7-9.1 us against 9.0-9.5 with the reads behind MFMAs 0-5 and the
// pieces behind 6, 9, .. 21 in six alternations; pieces first and reads last, or all pieces back to back: no
// faster; EXPERIMENTS.md)
constexpr int kKxRd0 = 1, kKxRdS = 2, kKxPc0 = 0, kKxPcS = 2;
// mfma6's (A plane, B plane) pairs in its order
constexpr int kM6A[6] = {2, 0, 1, 1, 0, 0}, kM6B[6] = {0, 2, 1, 0, 1, 0};
// output tile width (16 tiles per net, 8 splits of 512 rows at mb 4096); the
// pipelined body's register sets and gap table are laid out for 64
constexpr int kKxTW = 64;
template <int TW>
struct KxSmem {
  static constexpr int RUNS = 2 * 3 * 4, KG = TW * 16 + 16;     // runs per chunk (tensor x plane x row group), LDS bytes per run
  unsigned char ring[kKxD][RUNS][KG];
};
// the body of dw2_kx_kernel for workgroup b: the slab tile of (net, tile, split)
__device__ __forceinline__ void dw2_kx_body(int b, int mb, int S, int KR, int net_sel,
                                            const unsigned short* __restrict__ H1x,
                                            const unsigned short* __restrict__ dZ2x, float* __restrict__ p2,
                                            KxSmem<kKxTW>& sm) {
  constexpr int TW = kKxTW;
  static_assert(TW == 64, "one 1-KB piece per run, 2 x 2 tiles per wave");
  constexpr int H = 256, TT = H / TW, RUNS = KxSmem<TW>::RUNS;
  constexpr int XN = TW / 32, PW = RUNS / 4;                    // 16x16 tiles per wave side, pieces per wave
  constexpr int NM = 6 * XN * XN, NR = 6 * XN;                  // MFMAs and ds_read_b128 per wave and chunk
  // the gap table: read pair r behind MFMA kKxRd0 + r kKxRdS, piece k behind MFMA kKxPc0 + k kKxPcS
  static_assert(kKxRd0 + (NR / 2 - 1) * kKxRdS < NM && kKxPc0 + (PW - 1) * kKxPcS < NM, "gaps of one chunk");
  auto& ring = sm.ring;
  const int t = threadIdx.x, w = __builtin_amdgcn_readfirstlane(t >> 6), l = t & 63, li = l & 15, lg = l >> 4;
  const int s = b % S, tile = (b / S) % (TT * TT);
  const int net = net_sel < 0 ? b / (S * TT * TT) : net_sel;
  const int o0 = (tile / TT) * TW, n0 = (tile % TT) * TW;
  const int64_t PL = kx_rows(mb) * H;
  const int c_begin = s * (KR / 32), nch = (int)((min((int64_t)(s + 1) * KR, kx_rows(mb)) - (int64_t)s * KR) / 32);
  // piece k of wave w = run u = 4k + w (tensor k / 3, plane k % 3, row group w) of a chunk: 64 columns x 8
  // rows, 1 KB contiguous in the plane; its chunk-0 source (a scalar base, the lane's 16 B) is loop-invariant
  const unsigned short* src0[PW];
#pragma unroll
  for (int k = 0; k < PW; ++k) {
    const int u = 4 * k + w, tz = u / 12, p = (u / 4) % 3, q = u % 4;
    src0[k] = (tz == 0 ? dZ2x : H1x) + (int64_t)net * 3 * PL + p * PL +
              ((int64_t)(4 * c_begin + q) * H + (tz == 0 ? o0 : n0)) * 8;
  }
  auto piece = [&](int k, int c) {                                // this wave's piece k of chunk c
    __builtin_amdgcn_global_load_lds(src0[k] + (int64_t)c * (4 * H * 8) + (unsigned)(l * 8),
                                     (lds_void_t*)&ring[c % kKxD][4 * k + w][0], 16, 0, 0);
  };
  const int wo = w >> 1, wn = w & 1;
  // A[o][k] = dZ2[row 8lg + k'][o], B[k][n] = H1[row][n]: group lg of plane p
  const unsigned char* rdA = &ring[0][0 * 12 + lg][((TW / 2) * wo + li) * 16];
  const unsigned char* rdB = &ring[0][1 * 12 + lg][((TW / 2) * wn + li) * 16];
  // read j of a chunk, in the order the MFMAs first use them: plane pair j / (2 XN), then a[0], b[0], a[1], b[1]
  auto rd = [&](int j, int slot, s8v (&a)[XN][3], s8v (&bq)[XN][3]) {
    const int g = j / (2 * XN), x = (j % (2 * XN)) / 2;
    const int off = slot * (int)sizeof(ring[0]) + x * 256;
    if (j % 2 == 0) a[x][kM6A[g]] = *reinterpret_cast<const s8v*>(rdA + off + kM6A[g] * 4 * (int)sizeof(ring[0][0]));
    else bq[x][kM6B[g]] = *reinterpret_cast<const s8v*>(rdB + off + kM6B[g] * 4 * (int)sizeof(ring[0][0]));
  };
  f4 acc[XN][XN];
#pragma unroll
  for (int x = 0; x < XN; ++x)
#pragma unroll
    for (int y = 0; y < XN; ++y) acc[x][y] = f4{0.f, 0.f, 0.f, 0.f};
  // one iteration: chunk c from (a, bq), chunk c+1 into (na, nb), chunk c+kKxAhead into the ring
  auto iter = [&](int c, const s8v (&a)[XN][3], const s8v (&bq)[XN][3], s8v (&na)[XN][3], s8v (&nb)[XN][3]) {
    // vmcnt: this wave's pieces of chunk c+1 landed (younger: chunks c+2 .. c+kKxAhead-1, PW each);
    // lgkmcnt (kKxAhead == kKxD): its reads of chunk c, whose slot chunk c+kKxAhead takes, are done
    if constexpr (kKxAhead == kKxD) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"((kKxAhead - 2) * PW) : "memory");
    else asm volatile("s_waitcnt vmcnt(%0)" ::"n"((kKxAhead - 2) * PW) : "memory");
    __builtin_amdgcn_s_barrier();   // every wave's: chunk c+1 readable, the slot of chunk c+kKxAhead free
    const int cs = c + kKxAhead < nch ? c + kKxAhead : nch - 1;  // (tail: a harmless reload of the last chunk,
    const int rslot = (c + 1 < nch ? c + 1 : nch - 1) % kKxD;    //  and a re-read of it that nothing uses)
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < NM; ++i) {
      const int k = i / (XN * XN), x = (i / XN) % XN, y = i % XN;  // each accumulator: mfma6's six, in its order
      acc[x][y] = mfma_bf16(a[x][kM6A[k]], bq[y][kM6B[k]], acc[x][y]);
      __builtin_amdgcn_sched_barrier(0);
      if (i >= kKxRd0 && (i - kKxRd0) % kKxRdS == 0 && (i - kKxRd0) / kKxRdS < NR / 2) {
        rd(2 * ((i - kKxRd0) / kKxRdS), rslot, na, nb);
        rd(2 * ((i - kKxRd0) / kKxRdS) + 1, rslot, na, nb);
      }
      if (i >= kKxPc0 && (i - kKxPc0) % kKxPcS == 0 && (i - kKxPc0) / kKxPcS < PW) piece((i - kKxPc0) / kKxPcS, cs);
      __builtin_amdgcn_sched_barrier(0);
    }
    if (c + kKxAhead >= nch) __builtin_amdgcn_s_setprio(0);       // (the last chunk is staged)
  };
  // acc[x][y][q] = dW2[o0 + (TW/2)wo + 16x + 4lg + q][n0 + (TW/2)wn + 16y + li]; the address is formed here so
  // that no scalar load (of p2) is pending in the loop, where every LDS wait would wait for it too
  float* out = p2 + ((int64_t)net * S + s) * H * H;
  asm volatile("" : "+s"(out));
  s8v ra[2][XN][3], rb[2][XN][3];
#pragma unroll
  for (int c = 0; c < kKxAhead; ++c)
#pragma unroll
    for (int k = 0; k < PW; ++k) piece(k, c < nch ? c : nch - 1);
  // this wave's pieces of chunk 0 landed (younger: chunks 1 .. kKxAhead-1)
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"((kKxAhead - 1) * PW) : "memory");
  __builtin_amdgcn_s_barrier();                                   // every wave's
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    rd(j, 0, ra[0], rb[0]);
    __builtin_amdgcn_sched_barrier(0);                            // (in the loop's order)
  }
  for (int c = 0; c < nch; c += 2) {                              // (nch is the workgroup's: uniform branches)
    iter(c, ra[0], rb[0], ra[1], rb[1]);
    if (c + 1 >= nch) break;
    iter(c + 1, ra[1], rb[1], ra[0], rb[0]);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
  for (int x = 0; x < XN; ++x)
#pragma unroll
    for (int y = 0; y < XN; ++y)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        out[(int64_t)(o0 + (TW / 2) * wo + 16 * x + 4 * lg + q) * H + n0 + (TW / 2) * wn + 16 * y + li] = acc[x][y][q];
      }
}
template <int TW, bool SPAN = false>
__global__ void __launch_bounds__(256) dw2_kx_kernel(int mb, int S, int KR, int net_sel,
                                                     const unsigned short* __restrict__ H1x,
                                                     const unsigned short* __restrict__ dZ2x, float* __restrict__ p2,
                                                     unsigned long long* __restrict__ span) {
  const unsigned long long span_t0 = SPAN ? satrl_span::now() : 0ull;
  __shared__ __attribute__((aligned(16))) KxSmem<TW> sm;
  // at priority 3 until a wave has staged its last chunk (dw2_kx_body), as
  // the policy kernel: in-graph step 48.8 against 49.1 us at mb 4096 over
  // eight alternations on two boxes, equal (49.4) in three on a third;
  // bitwise the same (EXPERIMENTS.md round 5)
  __builtin_amdgcn_s_setprio(3);
  dw2_kx_body(blockIdx.x, mb, S, KR, net_sel, H1x, dZ2x, p2, sm);
  if constexpr (SPAN) satrl_span::exit(span, span_t0);
}
// split-K ways of dw2_kx_kernel: about kKxWgs workgroups, whole 32-row chunks,
// no empty split; half as many up to kKxHalfMb rows (mb 512: 4 splits of 128
// rows, in-graph step 28.2-28.8 against 29.2-29.3 us over three
// alternations -- a slower dW2, 3.3 against 2.5 us, but half the slabs for
// the reduce and the boundary before it; at mb 1024 slower, 37.2 against
// 35.6; EXPERIMENTS.md round 6)
constexpr int kKxWgs = 256, kKxHalfMb = 512;
int kx_tiles(int net) { return (net < 0 ? 2 : 1) * (256 / kKxTW) * (256 / kKxTW); }   // output tiles per split
int kx_splits(int mb, int net) {
  const int target = mb <= kKxHalfMb ? kKxWgs / 2 : kKxWgs;
  const int tiles = kx_tiles(net), nch = (int)(kx_rows(mb) / 32);
  int S = target / tiles;
  if (S > nch) S = nch;
  if (S < 1) S = 1;
  const int cps = (nch + S - 1) / S;                               // chunks per split
  return (nch + cps - 1) / cps;
}

// split-K ways of dw2_kernel: about kDwWgs workgroups, no empty split
constexpr int kDwWgs = 256;
int dw2_tiles(int H, int net) { return (net < 0 ? 2 : 1) * (H / 64) * (H / 64); }
int dw2_splits(int H, int mb, int net) {
  int S = kDwWgs / dw2_tiles(H, net);
  const int maxS = (mb + kDwKC - 1) / kDwKC;
  if (S > maxS) S = maxS;
  if (S < 1) S = 1;
  const int KR = ((mb + S - 1) / S + kDwKC - 1) / kDwKC * kDwKC;
  return (mb + KR - 1) / KR;                                     // no empty split
}

// ---------------------------------------------------------------------------
// reduce: sums the three partial-slab families into G (fixed order) and/or
// writes per-block squared norms per net (f64).  Everything moves as float4
// (every region boundary and slab stride is a multiple of 4 floats, and a
// float4 never straddles the actor/critic boundary).  Block ranges:
//   [0, nb2)          W2 region: 64 float4 columns x 4 chunks, S split-K slabs [2][S][H][H]
//   [nb2, nb2+nb1)    W1 region: 32 float4 columns x 8 chunks, nw1 slabs [nw1][2][H][20]
//   [nb2+nb1, ...)    tail: 8 float4 columns x 32 chunks, nwg slabs [nwg][6H+12]
// A chunk sums slabs c, c+CH, ... in that order, every load issued before the
// first add (one latency round), then chunk 0 adds the CH partials in order.
// ---------------------------------------------------------------------------
struct RedGeom { int nb2, nb1, nbt, S, nw1, nwg, net, ch2; };   // net: -1 both, 0 actor, 1 critic
__host__ __device__ inline int n_blocks_dev(const RedGeom& g) { return g.nb2 + g.nb1 + g.nbt; }
// chunks per column: W1, tail, W2 regions; the W2 region at H = 64 takes
// kRedCH2x chunks (its 128 one-block dW2 slabs per minibatch: 8 per thread,
// one load round, 16 float4 columns per block, 4x the blocks)
constexpr int kRedCH1 = 8, kRedCHt = 32, kRedCH2 = 4, kRedCH2x = 16;
__host__ __device__ inline int red_ch2(int H) { return H == 64 ? kRedCH2x : kRedCH2; }

__device__ __forceinline__ float4 f4add(float4 a, float4 b) {
  return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}
// IEEE division per component, as torch's G.div_(world) after the all-reduce
__device__ __forceinline__ float4 f4div(float4 a, float d) {
  return make_float4(a.x / d, a.y / d, a.z / d, a.w / d);
}
__device__ __forceinline__ double sq4(float4 v) {
  return (double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z + (double)v.w * v.w;
}

// s += part[w] for w = first, first + step, ... < nparts (at most NL terms), in
// that order: the NL loads go out first (clamped indices, so none is a branch)
// and the terms past nparts are selected to +0, so the sum is the plain loop's
// bit for bit (s starts at +0 and a round-to-nearest sum is never -0, so
// s + 0 == s).  (A runtime-trip loop unrolled by the compiler puts its
// remainder iterations in a prologue of one load, wait, add each: the tail
// region's four slabs per thread were four serial load round trips.)
template <int NL>
__device__ __forceinline__ void sum_strided4(float4& s, const float4* __restrict__ part, int64_t stride4,
                                             int first, int step, int nparts, int64_t col) {
  float4 v[NL];
#pragma unroll
  for (int i = 0; i < NL; ++i) v[i] = part[(int64_t)min(first + i * step, nparts - 1) * stride4 + col];
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int i = 0; i < NL; ++i) s = f4add(s, first + i * step < nparts ? v[i] : z);
}

template <int CH>
__device__ __forceinline__ float4 chunk_sum4(const float4* __restrict__ part, int64_t stride4, int nparts,
                                             int64_t col, bool valid, float4* red) {
  constexpr int EB = 256 / CH;
  const int t = threadIdx.x, e = t % EB, c = t / EB;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  if (valid && nparts > 0) {                                       // (the clamped index needs a slab)
    const int m = (nparts + CH - 1) / CH;                          // terms of the longest chunk (uniform)
    if (m <= 2) sum_strided4<2>(s, part, stride4, c, CH, nparts, col);
    else if (m <= 4) sum_strided4<4>(s, part, stride4, c, CH, nparts, col);
    else if (m <= 8) sum_strided4<8>(s, part, stride4, c, CH, nparts, col);
    else   // (H = 64's 128 dW2 slabs: two rounds of 16; one round of 32 measured 1.1 us slower)
      for (int w = c; w < nparts; w += 16 * CH) sum_strided4<16>(s, part, stride4, w, CH, nparts, col);
  }
  red[t] = s;
  __syncthreads();
  float4 tot = make_float4(0.f, 0.f, 0.f, 0.f);
  if (c == 0) {
    // the CH partials in order; their LDS reads go out 8 at a time ahead of
    // the adds (one read round trip per 8, not per 2)
    constexpr int KB = CH < 8 ? CH : 8;
#pragma unroll
    for (int k0 = 0; k0 < CH; k0 += KB) {
      float4 part[KB];
#pragma unroll
      for (int k = 0; k < KB; ++k) part[k] = red[(k0 + k) * EB + e];
#pragma unroll
      for (int k = 0; k < KB; ++k) tot = f4add(tot, part[k]);
    }
  }
  return tot;
}

// block-level f64 pair sum in fixed order, result in every thread
template <int CTRL>
__device__ __forceinline__ double dpp_d(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, false);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double lane_d(double v, int lane) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane),
                          __builtin_amdgcn_readlane(__double2loint(v), lane));
}
// wave sum of (a, c) in a fixed order: DPP sums of each 16-lane row (the
// row16_sum stages), then rows 0..3 by readlane -- no ds_bpermute round trips
__device__ __forceinline__ void wave_sum2(double& a, double& c) {
  a += dpp_d<0xB1>(a); c += dpp_d<0xB1>(c);
  a += dpp_d<0x4E>(a); c += dpp_d<0x4E>(c);
  a += dpp_d<0x141>(a); c += dpp_d<0x141>(c);
  a += dpp_d<0x140>(a); c += dpp_d<0x140>(c);
  a = ((lane_d(a, 0) + lane_d(a, 16)) + lane_d(a, 32)) + lane_d(a, 48);
  c = ((lane_d(c, 0) + lane_d(c, 16)) + lane_d(c, 32)) + lane_d(c, 48);
}
// (256-thread blocks: reduce, adam and the peer all-reduce.  The four wave
// pairs are read at once; a loop over blockDim's wave count was one LDS read
// round trip per wave)
__device__ __forceinline__ void block_sum2(double& a, double& c, double* sh) {
  constexpr int NW = 4;
  wave_sum2(a, c);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { sh[2 * w] = a; sh[2 * w + 1] = c; }
  __syncthreads();
  double v[2 * NW];
#pragma unroll
  for (int k = 0; k < 2 * NW; ++k) v[k] = sh[k];
  a = 0.0; c = 0.0;
#pragma unroll
  for (int k = 0; k < NW; ++k) { a += v[2 * k]; c += v[2 * k + 1]; }
}

// what a reduce thread ends with: the float4 of G it wrote (lead threads
// only: live), its float4 index in the flat layout, and its net
struct RedOut {
  float4 v;
  int64_t e4;
  int net;
  bool live;
};

// the W1 and tail parts of reduce (block b of the W1 region, or of the tail
// after it: b counts from the first W1 block): sums the rowpass slabs into G
// (mode & 1) or rescales G (world > 1), and adds this thread's squares to
// (sa, sc).
__device__ __forceinline__ void reduce_w1_tail(int H, const Layout& L, const RedGeom& g, int b, int mode,
                                               const float* __restrict__ p1, const float* __restrict__ pt,
                                               float4* __restrict__ G4, int world, float4* red, double& sa,
                                               double& sc, RedOut& o) {
  const int t = threadIdx.x;
  if (b < g.nb1) {                                                // W1: [nw1] slabs of 2*H*20
    constexpr int EB = 256 / kRedCH1;
    const int64_t n4 = 2LL * H * 20 / 4, h4 = (int64_t)H * 20 / 4;
    const int64_t col = (g.net > 0 ? h4 : 0) + (int64_t)b * EB + (t % EB);
    const bool valid = col < (g.net == 0 ? h4 : n4), lead = t < EB;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (mode & 1) {
      v = chunk_sum4<kRedCH1>(reinterpret_cast<const float4*>(p1), n4, g.nw1, col, valid, red);
      if (lead && valid) G4[L.W1 / 4 + col] = v;
    } else if (lead && valid) {
      v = G4[L.W1 / 4 + col];
      if (world > 1) { v = f4div(v, (float)world); G4[L.W1 / 4 + col] = v; }
    }
    if (lead && valid) {                                          // (selects, not a pointer to sa / sc)
      const double q = sq4(v);
      const bool crit = col * 4 >= (int64_t)H * 20;
      sa += crit ? 0.0 : q;
      sc += crit ? q : 0.0;
    }
    o = RedOut{v, L.W1 / 4 + col, col * 4 >= (int64_t)H * 20 ? 1 : 0, lead && valid};
  } else {                                                        // tail: [nwg] slabs of 6H+12
    b -= g.nb1;
    constexpr int EB = 256 / kRedCHt;
    const int64_t n4 = L.tail / 4, col = (int64_t)b * EB + (t % EB);
    const bool valid = col < n4 && (g.net < 0 || net_of(L, L.b2 + col * 4, H) == g.net), lead = t < EB;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (mode & 1) {
      v = chunk_sum4<kRedCHt>(reinterpret_cast<const float4*>(pt), n4, g.nwg, col, valid, red);
      if (lead && valid) G4[L.b2 / 4 + col] = v;
    } else if (lead && valid) {
      v = G4[L.b2 / 4 + col];
      if (world > 1) { v = f4div(v, (float)world); G4[L.b2 / 4 + col] = v; }
    }
    const bool crit = valid && net_of(L, L.b2 + col * 4, H);
    if (lead && valid) {
      const double q = sq4(v);
      sa += crit ? 0.0 : q;
      sc += crit ? q : 0.0;
    }
    o = RedOut{v, L.b2 / 4 + col, crit ? 1 : 0, lead && valid};
  }
}

// block b of reduce: the W2 region, else the W1 / tail regions
__device__ __forceinline__ void reduce_block(int H, const Layout& L, const RedGeom& g, int b, int mode,
                                             const float* __restrict__ p2, const float* __restrict__ p1,
                                             const float* __restrict__ pt, float4* __restrict__ G4, int world,
                                             float4* red, double& sa, double& sc, RedOut& o) {
  const int t = threadIdx.x;
  const int64_t HH4 = (int64_t)H * H / 4;
  if (b < g.nb2) {                                                // W2: [2][S] split-K slabs of H*H
    const int EB = 256 / g.ch2;
    const int64_t col = (g.net > 0 ? HH4 : 0) + (int64_t)b * EB + (t % EB);
    const bool valid = col < (g.net < 0 ? 2 : g.net + 1) * HH4, lead = t < EB;
    const int net = col >= HH4;                                   // EB divides HH4: one net per block
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (mode & 1) {
      const float4* p2n = reinterpret_cast<const float4*>(p2) + (int64_t)net * g.S * HH4;
      v = g.ch2 == kRedCH2x ? chunk_sum4<kRedCH2x>(p2n, HH4, g.S, col - net * HH4, valid, red)
                            : chunk_sum4<kRedCH2>(p2n, HH4, g.S, col - net * HH4, valid, red);
      if (lead && valid) G4[col] = v;
    } else if (lead && valid) {
      v = G4[col];
      if (world > 1) { v = f4div(v, (float)world); G4[col] = v; }
    }
    if (lead && valid) {
      if (net) sc += sq4(v); else sa += sq4(v);
    }
    o = RedOut{v, col, net, lead && valid};
  } else {
    reduce_w1_tail(H, L, g, b - g.nb2, mode, p1, pt, G4, world, red, sa, sc, o);
  }
}

template <bool SPAN = false>
__global__ void __launch_bounds__(256) reduce_kernel(int H, int mode, int nb2, int S, int net_sel, int ch2,
                                                     const float* __restrict__ p2, double* __restrict__ steps,
                                                     float* __restrict__ G, double* __restrict__ nsq, RedGeom g,
                                                     const float* __restrict__ p1, const float* __restrict__ pt,
                                                     int world, unsigned long long* __restrict__ span) {
  const unsigned long long span_t0 = SPAN ? satrl_span::now() : 0ull;
  // (argument order: the 14 dwords up to nsq are preloaded.  A by-value struct
  // is never preloaded, so what a W2 block -- every block of the update's
  // reduce launch -- reads of the geometry comes as scalars ahead of it, and
  // g's copies of them are replaced: its slab loads wait for no s_load)
  g.nb2 = nb2; g.S = S; g.net = net_sel; g.ch2 = ch2;
  const Layout L = layout(H);
  __shared__ double sh[8];
  __shared__ float4 red[256];
  double sa = 0.0, sc = 0.0;
  const int t = threadIdx.x;
  float4* G4 = reinterpret_cast<float4*>(G);
  // the step counters, read before the slab loads (read at the end they were
  // one more load round trip on block 0's path), advanced at the end
  double st0 = 0.0, st1 = 0.0;
  if ((mode & 2) && blockIdx.x == 0 && t == 0) { st0 = steps[0]; st1 = steps[1]; }
  RedOut o;
  reduce_block(H, L, g, blockIdx.x, mode, p2, p1, pt, G4, world, red, sa, sc, o);
  if (mode & 2) {
    block_sum2(sa, sc, sh);
    if (t == 0) {
      nsq[2 * blockIdx.x] = sa;
      nsq[2 * blockIdx.x + 1] = sc;
      if (blockIdx.x == 0) {
        if (g.net != 1) steps[0] = st0 + 1.0;
        if (g.net != 0) steps[1] = st1 + 1.0;
      }
    }
  }
  if constexpr (SPAN) satrl_span::exit(span, span_t0);
}

// dw2_kx and the reduce's W1 / tail regions in one launch
// (satrl_ppo_dw2_kx_w1): blocks [0, ndw) are dw2_kx_kernel's, the rest
// reduce_kernel's W1 / tail blocks.  Their slabs are the rowpass's (ready when
// this launch starts), so they run beside the dW2 stream instead of on the
// reduce's critical path; they write G's W1 / tail regions and (mode & 2)
// their squared-norm pairs at the reduce's own block indices, and
// satrl_ppo_reduce with mode bit 4 then runs the W2 blocks only.  Same code,
// same order: bitwise the two launches' G and norms.
template <int TW, bool SPAN = false>
__global__ void __launch_bounds__(256) dw2_kx_w1_kernel(int mb, int S, int KR, int net_sel,
                                                        const unsigned short* __restrict__ H1x,
                                                        const unsigned short* __restrict__ dZ2x, float* __restrict__ p2,
                                                        int ndw, RedGeom g, int mode, const float* __restrict__ p1,
                                                        const float* __restrict__ pt, float* __restrict__ G,
                                                        double* __restrict__ nsq, unsigned long long* __restrict__ span) {
  // (argument order: the 11 dwords up to ndw are preloaded -- all a dW2
  // block's plane stream needs; a by-value struct ends the preloaded run, and
  // the few reduce blocks behind it run beside the stream, off its path)
  const unsigned long long span_t0 = SPAN ? satrl_span::now() : 0ull;
  __shared__ __attribute__((aligned(16))) KxSmem<TW> sm;
  if ((int)blockIdx.x < ndw) {
    __builtin_amdgcn_s_setprio(3);                               // (as dw2_kx_kernel)
    dw2_kx_body(blockIdx.x, mb, S, KR, net_sel, H1x, dZ2x, p2, sm);
  } else {
    // the reduce block's LDS (its float4 chunk sums, the block's norm pair)
    // inside the ring, which no block of this kind uses
    static_assert(sizeof(KxSmem<TW>) >= 256 * sizeof(float4) + 8 * sizeof(double), "reduce LDS in the ring");
    float4* red = reinterpret_cast<float4*>(&sm.ring[0][0][0]);
    double* sh = reinterpret_cast<double*>(reinterpret_cast<unsigned char*>(&sm.ring[0][0][0]) + 256 * sizeof(float4));
    const int b = (int)blockIdx.x - ndw;
    double sa = 0.0, sc = 0.0;
    RedOut o;
    reduce_w1_tail(256, layout(256), g, b, mode, p1, pt, reinterpret_cast<float4*>(G), 1, red, sa, sc, o);
    if (mode & 2) {
      block_sum2(sa, sc, sh);
      if (threadIdx.x == 0) {
        nsq[2 * (g.nb2 + b)] = sa;
        nsq[2 * (g.nb2 + b) + 1] = sc;
      }
    }
  }
  if constexpr (SPAN) satrl_span::exit(span, span_t0);
}

// ---------------------------------------------------------------------------
// adam: torch.nn.utils.clip_grad_norm_ + torch.optim.Adam (_single_tensor_adam)
// Every block first folds the per-block norms (fixed order, identical in
// every block).  Blocks [0, nbw): one 32x32 tile of a net's fc2.weight each,
// float4 per thread, and the updated tile goes out transposed through LDS
// into W2T (coalesced).  Blocks [nbw, ...): the rest of the layout, float4.
// ---------------------------------------------------------------------------
// The updated 32x32 tile tb of net's fc2.weight (thread t holds row n0 + t/8,
// columns k0 + (t%8)*4 .. +3 in v) into the fc2 operand image, the f32
// transpose (through LDS, so every store is coalesced).  Every thread of the
// block calls it.
__device__ __forceinline__ void w2x_tile(int H, int net, int tb, float4 v, void* __restrict__ W2X,
                                         float (&tile)[32][33]) {
  const int t = threadIdx.x, nl = t >> 3, kl = (t & 7) * 4, ntc = H / 32;
  const int n0 = (tb / ntc) * 32, k0 = (tb % ntc) * 32;
  const int64_t HH = (int64_t)H * H;
  tile[nl][kl] = v.x; tile[nl][kl + 1] = v.y; tile[nl][kl + 2] = v.z; tile[nl][kl + 3] = v.w;
  __syncthreads();
  // W2T[net][k0 + t/8][n0 + (t%8)*4 + q] = W2[net][n0 + (t%8)*4 + q][k0 + t/8]
  const float4 o = make_float4(tile[kl][nl], tile[kl + 1][nl], tile[kl + 2][nl], tile[kl + 3][nl]);
  reinterpret_cast<float4*>(W2X)[((int64_t)net * HH + (int64_t)(k0 + nl) * H + n0 + kl) / 4] = o;
}

// the fc2 operand image of P (satrl_ppo_w2x_sync): adam_kernel's W2 blocks
// without the step
__global__ void __launch_bounds__(256) w2x_sync_kernel(int H, int net_sel, const float* __restrict__ P,
                                                       void* __restrict__ W2X) {
  __shared__ float tile[32][33];
  const int t = threadIdx.x, ntc = H / 32, tb = blockIdx.x % (ntc * ntc);
  const int net = net_sel < 0 ? (int)(blockIdx.x / (ntc * ntc)) : net_sel;
  const int n = (tb / ntc) * 32 + (t >> 3), k = (tb % ntc) * 32 + (t & 7) * 4;
  const float4 v = *reinterpret_cast<const float4*>(P + (int64_t)net * H * H + (int64_t)n * H + k);
  w2x_tile(H, net, tb, v, W2X, tile);
}

__device__ __forceinline__ float adam_elem(float g, float& m, float& v, float p, float coef, float step_size,
                                           float bc2s, float w1, float w2, float beta2, float eps, int use_clip) {
  if (use_clip) g = g * coef;                                      // grads.mul_(clip_coef_clamped)
  m = m + w1 * (g - m);                                            // exp_avg.lerp_(grad, 1 - beta1)
  v = v * beta2 + w2 * (g * g);                                    // mul_(beta2).addcmul_(g, g, 1 - beta2)
  const float denom = sqrtf(v) / bc2s + eps;
  return p + (-step_size) * (m / denom);                           // addcdiv_(m, denom, -step_size)
}

template <bool SPAN = false>
__global__ void __launch_bounds__(256) adam_kernel(int H, int nblk, const double* __restrict__ nsq,
                                                   const float* __restrict__ G, float* __restrict__ P,
                                                   float* __restrict__ M, float* __restrict__ V, int net_sel,
                                                   int bct_len, const double* __restrict__ steps,
                                                   const double* __restrict__ bct, const float* __restrict__ lr,
                                                   float beta1, float beta2, float eps, float max_norm, int use_clip,
                                                   void* __restrict__ W2X, unsigned long long* __restrict__ span) {
  // (argument order: the 14 dwords up to bct_len are preloaded -- the norm
  // partials' and the G / M / V / P loads below need nothing else)
  const unsigned long long span_t0 = SPAN ? satrl_span::now() : 0ull;
  const Layout L = layout(H);
  __shared__ double sh[8];
  __shared__ float tile[32][33];
  const int t = threadIdx.x;
  const int ntc = H / 32, nbw = (net_sel < 0 ? 2 : 1) * ntc * ntc;
  // this thread's element (float4) and net, and whether it has one
  int64_t e4;
  int net;
  bool live = true;
  if ((int)blockIdx.x < nbw) {
    const int tb = blockIdx.x % (ntc * ntc);
    net = net_sel < 0 ? (int)(blockIdx.x / (ntc * ntc)) : net_sel;
    const int n = (tb / ntc) * 32 + (t >> 3), k = (tb % ntc) * 32 + (t & 7) * 4;
    e4 = ((int64_t)net * H * H + (int64_t)n * H + k) / 4;
  } else {
    e4 = L.W1 / 4 + (int64_t)(blockIdx.x - nbw) * 256 + t;
    live = e4 < L.total / 4;
    net = live ? net_of(L, e4 * 4, H) : 0;
    live = live && (net_sel < 0 || net == net_sel);
  }
  // the norm partials' loads go out first, this thread's G/M/V/P right
  // behind them: the fold below waits only for the partials (vmcnt is in
  // order), so the operand latency overlaps the fold
  // (all loads unconditional on clamped indices, so none becomes a branch)
  const double2* nsq2 = reinterpret_cast<const double2*>(nsq);
  double2 pn2[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) pn2[i] = nsq2[min(t + 256 * i, nblk - 1)];
  const float4* G4 = reinterpret_cast<const float4*>(G);
  float4* P4 = reinterpret_cast<float4*>(P);
  float4* M4 = reinterpret_cast<float4*>(M);
  float4* V4 = reinterpret_cast<float4*>(V);
  const int64_t el = live ? e4 : 0;
  const float4 g = G4[el];
  float4 m = M4[el], v = V4[el];
  const float4 p = P4[el];
  // both nets' step counts, learning rates and bias-correction rows, issued
  // here too: after the fold (a barrier the compiler does not hoist loads
  // over) they were two dependent load round trips on the kernel's path
  const double st_a = steps[0], st_c = steps[1];
  const float lr_a = lr[0], lr_c = lr[1];
  const int ka = (int)st_a, kc = (int)st_c;
  const double2* bct2 = reinterpret_cast<const double2*>(bct);
  const double2 bca = bct2[ka < bct_len ? ka : bct_len - 1], bcc = bct2[kc < bct_len ? kc : bct_len - 1];
  double a = 0.0, c = 0.0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {                                    // k = t, t+256, ... in order, as the loop
    // x * 1.0 == x, x * 0.0 + a == a for these non-negative sums: bitwise the
    // loop's skip, without a branch the compiler would sink the load into
    const double in = t + 256 * i < nblk ? 1.0 : 0.0;
    a += pn2[i].x * in;
    c += pn2[i].y * in;
  }
  if (nblk > 1024) {                                               // (not at the sizes in use)
    for (int k = t + 1024; k < nblk; k += 256) { a += nsq[2 * k]; c += nsq[2 * k + 1]; }
  }
  block_sum2(a, c, sh);
  // every thread folds the same partials in the same order, so each derives
  // its own net's constants (no second barrier)
  float coef, ss, b2s;
  {
    const double nn = net == 0 ? a : c;
    const float nrm = (float)sqrt(nn);
    coef = use_clip ? fminf(max_norm / (nrm + 1e-6f), 1.0f) : 1.0f;
    // bct[2*step] = 1 - beta1**step, bct[2*step+1] = sqrt(1 - beta2**step) (python float
    // math, as torch.optim.Adam computes them); constant 1.0 past the table
    const int st = net == 0 ? ka : kc;
    const double2 bc = net == 0 ? bca : bcc;
    const double bc1 = st < bct_len ? bc.x : 1.0;
    const double bc2s = st < bct_len ? bc.y : 1.0;
    ss = (float)((double)(net == 0 ? lr_a : lr_c) / bc1);
    b2s = (float)bc2s;
  }
  const float w1 = (float)(1.0 - (double)beta1);                  // lerp weight 1 - beta1
  const float w2 = (float)(1.0 - (double)beta2);
  if (!live) {                                                     // (W1.. tail blocks only: no barrier follows)
    if constexpr (SPAN) satrl_span::exit(span, span_t0);
    return;
  }
  float4 pn;
  pn.x = adam_elem(g.x, m.x, v.x, p.x, coef, ss, b2s, w1, w2, beta2, eps, use_clip);
  pn.y = adam_elem(g.y, m.y, v.y, p.y, coef, ss, b2s, w1, w2, beta2, eps, use_clip);
  pn.z = adam_elem(g.z, m.z, v.z, p.z, coef, ss, b2s, w1, w2, beta2, eps, use_clip);
  pn.w = adam_elem(g.w, m.w, v.w, p.w, coef, ss, b2s, w1, w2, beta2, eps, use_clip);
  P4[e4] = pn;
  M4[e4] = m;
  V4[e4] = v;
  if ((int)blockIdx.x < nbw && W2X != nullptr)                     // keep the fc2 operand image current
    w2x_tile(H, net, blockIdx.x % (ntc * ntc), pn, W2X, tile);
  if constexpr (SPAN) satrl_span::exit(span, span_t0);
}

// ---------------------------------------------------------------------------
// stage: the rows of a group of minibatches gathered contiguously, at the
// permutation offset a device counter holds (8 lanes x float4 per 128-B row)
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) stage_kernel(int64_t rows, const float4* __restrict__ src,
                                                    const int64_t* __restrict__ perm,
                                                    const int64_t* __restrict__ group, float4* __restrict__ stage) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, r = t >> 3;
  if (r >= rows) return;
  const int64_t row = perm[group[0] * rows + r];
  stage[t] = src[row * 8 + (t & 7)];
}

__global__ void group_advance_kernel(int64_t* group) { group[0] += 1; }

__global__ void __launch_bounds__(256) tanh_kernel(int64_t n, const float* __restrict__ x, float* __restrict__ y) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) y[i] = tanh_f32(x[i]);
}

// test entry (satrl_tanh_forms): thread i takes x[8i .. 8i+7], a call site's
// eight values; FORM 0: tanh_f32 on each, FORM 1: tanh_f32_n on the eight
template <int FORM>
__global__ void __launch_bounds__(256) tanh_forms_kernel(int64_t n8, const float* __restrict__ x,
                                                         float* __restrict__ y) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n8) return;
  float v[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) v[q] = x[8 * i + q];
  if constexpr (FORM == 1) {
    tanh_f32_n(v);
  } else {
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = tanh_f32(v[q]);
  }
#pragma unroll
  for (int q = 0; q < 8; ++q) y[8 * i + q] = v[q];
}

// rows per rowpass workgroup for a minibatch of mb rows: kRowsShort at
// H = 256 up to kShortMb rows (twice the workgroups on the chip; measured
// faster up to mb 1024, even at 2048, slower at 4096: DESIGN.md §3.4)
constexpr int kShortMb = 1024;
int short_mb() { return kShortMb; }
int rows_per_wg(int H, int mb) {
  return (H == 256 && kRows == 32 && mb <= short_mb()) ? kRowsShort : kRows;
}
int n_head_wg(int H, int mb) {
  const int R = rows_per_wg(H, mb);
  return (mb + R - 1) / R;
}
int n_w1_wg(int H, int mb) { return n_head_wg(H, mb); }
// slab capacity a minibatch of mb rows needs, and any shorter one (a ragged
// tail of a minibatch above the short threshold can have more row blocks)
int n_head_wg_cap(int H, int mb) {
  const int m = mb < short_mb() ? mb : short_mb();
  const int a = n_head_wg(H, mb), b = m > 0 ? n_head_wg(H, m) : 0;
  return a > b ? a : b;
}
RedGeom geom(int H, int mb, int S, int net = -1) {
  const Layout L = layout(H);
  const int nn = net < 0 ? 2 : 1;                                  // nets covered
  RedGeom g;
  g.ch2 = red_ch2(H);
  g.nb2 = (int)((nn * (int64_t)H * H / 4 + (256 / g.ch2) - 1) / (256 / g.ch2));
  g.nb1 = (int)((nn * (int64_t)H * 20 / 4 + (256 / kRedCH1) - 1) / (256 / kRedCH1));
  g.nbt = (int)((L.tail / 4 + (256 / kRedCHt) - 1) / (256 / kRedCHt));
  g.S = S;
  g.nw1 = n_w1_wg(H, mb);
  g.nwg = n_head_wg(H, mb);
  g.net = net;
  return g;
}
int n_blocks(const RedGeom& g) { return g.nb2 + g.nb1 + g.nbt; }
int n_adam_blocks(int H, int net) {
  const Layout L = layout(H);
  return (net < 0 ? 2 : 1) * (H / 32) * (H / 32) + (int)(((L.total - L.W1) / 4 + 255) / 256);
}

bool valid_h(int H) { return H == 64 || H == 128 || H == 256; }

// What every entry point below takes its refusals, width dispatch and launch
// check from.  A refusal is satrl_error.h's fail(code, entry point, reason); the
// entry point passes __func__, also to a checker or launcher it shares with others.
using satrl_err::fail;
using satrl_err::grid_of;
using satrl_err::launch;
using satrl_err::launched;
using satrl_err::null_arg;
using std::to_string;

// A width as its compile-time pair: f(Width<H, waves per workgroup>{}) of a
// validated H.  The H 256 wave count belongs to the kernel family, so the call
// site states it (kPolNW: policy / diagnostics, kNW256: rowpass).
template <int H_, int NW_>
struct Width { static constexpr int H = H_, NW = NW_; };
template <int NW256, class F>
auto with_width(int H, F&& f) {
  if (H == 64) return f(Width<64, 4>{});
  if (H == 128) return f(Width<128, 8>{});
  return f(Width<256, NW256>{});
}
template <int NW256>
int waves_of(int H) { return with_width<NW256>(H, [](auto w) { return decltype(w)::NW; }); }

// a scalar argument outside lo .. hi, refused under its name
int outside(const char* who, const char* name, int64_t v, int64_t lo, int64_t hi) {
  if (v >= lo && v <= hi) return 0;
  return fail(-1, who, name + (" " + to_string(v)) + " is outside " + to_string(lo) + " .. " + to_string(hi));
}
// The refusals the width-taking entry points share, in this order; 0 when none
// applies.  `widths` is the set the entry point takes, as the OR of them; `n`
// its row count under its own name (1 where it has none); `net` 0 where it has none.
constexpr int kAnyH = 64 | 128 | 256, kFusedH = 64 | 128;
int refuse(const char* who, int H, int widths, int64_t n, const char* n_name, int net,
           const satrl_err::Ptrs& need = {"", {}}) {
  if (!valid_h(H) || !(H & widths))
    return fail(-1, who, "H " + to_string(H) + " is not " +
                             (widths == kAnyH ? "64/128/256" : widths == kFusedH ? "64/128" : "256"));
  if (n <= 0) return fail(-1, who, std::string(n_name) + " " + to_string(n) + " is empty (<= 0)");
  if (int rc = outside(who, "net", net, -1, 1)) return rc;
  return null_arg(who, need);
}

// Caller-buffer capacity checks of the C-ABI (before any launch).  A one-net
// call (net 1) addresses the second half of a [2][...] buffer, so only net 0
// may pass half the size.
int64_t nets_span(int net) { return net == 0 ? 1 : 2; }
// p2 [2][S][H][H] f32 split-K slabs
int p2_fits(const char* who, int H, int net, int S, int64_t p2_floats) {
  const int64_t need = nets_span(net) * (int64_t)S * H * H;
  if (p2_floats >= need) return 0;
  return fail(-1, who, "p2 holds " + to_string(p2_floats) + " floats, " + to_string(S) + " splits need " +
                           to_string(need));
}
// the k-packed planes u16 [2][3][kx_rows(mb)][H] (satrl_ppo_kx_elems)
int kx_fits(const char* who, int H, int mb, int net, int64_t kx_elems) {
  const int64_t need = nets_span(net) * 3 * kx_rows(mb) * H;
  if (kx_elems >= need) return 0;
  return fail(-1, who, "the H1x / dZ2x planes hold " + to_string(kx_elems) + " elements, mb " +
                           to_string(mb) + " needs " + to_string(need));
}
// *per: the rows one of S splits of `rows` takes, a multiple of `round`; no split may be empty
int split_size(const char* who, int S, int rows, int round, const char* query, int* per) {
  if (S < 1) return fail(-1, who, "S " + to_string(S) + " < 1");
  *per = ((rows + S - 1) / S + round - 1) / round * round;
  if ((int64_t)*per * (S - 1) < rows) return 0;
  return fail(-1, who, to_string(S) + " splits leave an empty split: use " + query);
}
// Workgroups of kernel k at `threads` threads that can be resident at once on
// the current device, CUs x workgroups per CU; false when a query fails.
struct Residency {
  int cus = 0, per_cu = 0;
  int blocks() const { return cus * per_cu; }
};
template <class K>
bool residency(K k, int threads, Residency* r) {
  int dev = 0;
  return hipGetDevice(&dev) == hipSuccess &&
         hipDeviceGetAttribute(&r->cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess &&
         hipOccupancyMaxActiveBlocksPerMultiprocessor(&r->per_cu, k, threads, 0) == hipSuccess;
}

using satrl_span::launch_span;
// policy_kernel<H, NW, MODE> over N rows of `nag` agents, probed as span kind `kind`
template <int MODE, class... A>
int launch_policy(const char* who, int H, int kind, int nag, int64_t N, void* stream, A... args) {
  dim3 g;
  if (int rc = grid_of(who, nag * ((N + kPolRows - 1) / kPolRows), &g)) return rc;
  with_width<kPolNW>(H, [&](auto w) {
    using W = decltype(w);
    launch_span(policy_kernel<W::H, W::NW, MODE, true>, policy_kernel<W::H, W::NW, MODE>,
                satrl_span::take(kind, (int64_t)g.x * W::NW), g, dim3(W::NW * 64), stream, N, args...);
  });
  return launched(who);
}
// the two Philox keys of both agents' action streams
struct PolicyKeys {
  uint32_t k00, k01, k10, k11;
  explicit PolicyKeys(uint64_t seed) {
    philox_key(seed, 0, k00, k01);
    philox_key(seed, 1, k10, k11);
  }
};
// the launch of both fused forms (MODE 0: act + logp, MODE 2: actions only)
template <int MODE>
int launch_policy_scripted(const char* who, int H, int64_t N, const float* obs, const float* obs_law,
                           const float* P, int agent, float max_action, int det, uint64_t seed, int64_t env_offset,
                           uint64_t step, const uint64_t* step_base, float* act, float* logp,
                           const satrl_scripted_law* law, float* act_scripted, void* stream) {
  if (int rc = refuse(who, H, kAnyH, N, "N", 0, SATRL_PTRS(obs, P, act))) return rc;
  if (MODE == 0 && !logp) return fail(-1, who, "logp is NULL");
  if (!obs_law || !law || !act_scripted) return fail(-1, who, "a NULL obs_law, law or act_scripted");
  if (agent != 0 && agent != 1) return fail(-1, who, "agent is 0 or 1");
  if (det != 0 && det != 1) return fail(-1, who, "det is 0 or 1");
  uint32_t k0, k1;
  philox_key(seed, (uint32_t)agent, k0, k1);                       // the learner's own key stream
  const int64_t nblk = (N + kPolRows - 1) / kPolRows;
  return with_width<kPolNW>(H, [&](auto w) {
    constexpr int NT = decltype(w)::NW * 64;                       // the law's rows: one per thread of the tail blocks
    return launch(who, policy_scripted_kernel<decltype(w)::H, decltype(w)::NW, MODE>, nblk + (N + NT - 1) / NT, NT,
                  stream, N, obs, P, obs_law, law, act_scripted, (int)nblk, max_action, k0, k1, env_offset, step,
                  step_base, act, logp, det);
  });
}

// the two instantiations of a rowpass_kernel, {probed, plain}
template <int H, int NW, int R, bool FDW2, bool KX, bool HANDOFF = false>
auto rowpass_k() {
  return std::make_pair(rowpass_kernel<H, NW, R, FDW2, KX, HANDOFF, true>, rowpass_kernel<H, NW, R, FDW2, KX, HANDOFF>);
}

// ---------------------------------------------------------------------------
// peer_allreduce: the data-parallel gradient all-reduce of G over the W ranks
// of one node without RCCL, fused with reduce_dp (G /= W, the per-block
// squared norms, the step counters).  Each rank owns an exchange buffer that
// every peer has mapped (IPC, uncached device memory); a value travels as
// an 8-B granule {tag, f32} written by ONE 8-B system-scope store, so the
// reader polls the granule itself -- no flag, no fence, no barrier
// (MI355X_MICROARCH.md "Valid forms", the granule form).  Two shots:
//   1 reduce-scatter push: every element goes to the rank that owns its
//     slice (slice j = elements [j*sl, (j+1)*sl)), slot [this rank];
//   2 the owner sums slot 0, 1, ... W-1 of each of its elements in rank
//     order, divides by W (IEEE, as reduce_dp) and pushes the result to
//     every rank's gather slot [owner];
//   3 every rank polls its gather slots into G.
// Each slice is summed once, in rank order, then broadcast, so every rank
// gets identical bits (and, at W = 2, the bits of c10d's SUM / 2).  Phase
// 3 hands out G exactly as reduce_kernel's blocks do (a float4 per lead
// thread of each of reduce_dp's blocks), so nsq is bitwise reduce_dp's.
// The grid is at most one workgroup per CU (satrl_ppo_allreduce_peer checks
// that every block is resident): a block takes reduce_dp's blocks
// blockIdx.x, + gridDim.x, ... in turn, so its spinning waves leave every CU
// room for the kernels of other streams or of a rank sharing the device.
// The tag is the call count: block b keeps its own counter in this rank's
// buffer and every call advances every counter once, on every rank (the
// grid size must be the same on every rank).  Waits are bounded (the
// caller's deadline in s_memrealtime ticks): a peer that never pushes sets
// the error word instead of hanging the GPU; satrl_peer_reset re-arms the
// counters and the word once every rank has stopped.
// ---------------------------------------------------------------------------
constexpr int kPeerMaxW = 8, kPeerMaxBlocks = 1024;
constexpr int64_t kPeerHdr = 4 * kPeerMaxBlocks + 256;           // epoch counters, error word
struct PeerBufs {
  unsigned long long* buf[kPeerMaxW];                              // every rank's buffer (this rank's own too)
};
typedef __attribute__((address_space(1))) unsigned long long gu64;
typedef __attribute__((address_space(1))) unsigned int gu32;

__host__ __device__ inline int64_t peer_slice(int64_t n, int world) { return (n + world - 1) / world; }
__host__ __device__ inline int64_t peer_bytes(int64_t n, int world) {
  return kPeerHdr + 2 * (int64_t)world * peer_slice(n, world) * 8;
}

__device__ __forceinline__ void peer_push(unsigned long long* base, int64_t word, unsigned tag, float v) {
  __hip_atomic_store((gu64*)(base) + word, ((unsigned long long)tag << 32) | __float_as_uint(v), __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_SYSTEM);
}
// the sticky error word of a rank's buffer (after the per-block counters)
__device__ __forceinline__ gu64* peer_err_word(unsigned long long* base) {
  return (gu64*)(base) + (4 * kPeerMaxBlocks) / 8;
}
// the value of a granule once its tag is `tag` (bounded wait: once a wait of
// this thread has run out, the rest return at once, the call being invalid).
// Every 16th poll also reads this rank's own error word (`mine`): a peer that
// gave up sets it in every rank's buffer, so the survivors fail fast instead
// of spending their own deadline
__device__ __forceinline__ float peer_pull(const unsigned long long* base, int64_t word, unsigned tag,
                                           unsigned long long* mine, unsigned long long t0,
                                           unsigned long long ticks, bool& ok) {
  const gu64* g = (const gu64*)(base) + word;
  unsigned long long x = __hip_atomic_load(g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  unsigned polls = 0;
  while (ok && (unsigned)(x >> 32) != tag) {
    if (__builtin_amdgcn_s_memrealtime() - t0 > ticks) { ok = false; break; }   // 100 MHz ticks
    if ((++polls & 15u) == 0 &&
        __hip_atomic_load(peer_err_word(mine), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0ull) {
      ok = false;
      break;
    }
    __builtin_amdgcn_s_sleep(1);
    x = __hip_atomic_load(g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  return __uint_as_float((unsigned)x);
}

// the float4 of G reduce_dp's block rb hands thread t (its lead threads), or -1
__device__ __forceinline__ int64_t peer_col(const Layout& L, const RedGeom& g, int H, int rb, int t) {
  if (rb < g.nb2) return t < 256 / g.ch2 ? (int64_t)rb * (256 / g.ch2) + t : -1;
  if (rb < g.nb2 + g.nb1) {
    const int64_t c = (int64_t)(rb - g.nb2) * (256 / kRedCH1) + t;
    return t < 256 / kRedCH1 && c < 2LL * H * 20 / 4 ? L.W1 / 4 + c : -1;
  }
  const int64_t c = (int64_t)(rb - g.nb2 - g.nb1) * (256 / kRedCHt) + t;
  return t < 256 / kRedCHt && c < L.tail / 4 ? L.b2 / 4 + c : -1;
}

__global__ void __launch_bounds__(256) peer_allreduce_kernel(int H, RedGeom g, int world, int rank, PeerBufs pb,
                                                             float* __restrict__ G, double* __restrict__ nsq,
                                                             double* __restrict__ steps,
                                                             unsigned long long ticks) {
  const Layout L = layout(H);
  __shared__ double sh[8];
  __shared__ unsigned tag_s;
  const int t = threadIdx.x, b = blockIdx.x, nb = gridDim.x, nred = n_blocks_dev(g);
  const int64_t n = L.total, sl = peer_slice(n, world);
  unsigned long long* mine = pb.buf[rank];
  const int64_t rs = kPeerHdr / 8, ag = rs + (int64_t)world * sl;  // word offsets of the two slot arrays
  __shared__ int failed_s;
  if (t == 0) {                                                    // this call's tag: block b's counter + 1
    // a failed call earlier (this rank's or a peer's: the word is set in every
    // buffer) makes every later call return at once -- the update is invalid
    // until PeerComm.reset, and the calls queued behind the failure (up to a
    // graph group of them) must not each spend the deadline again
    failed_s = __hip_atomic_load(peer_err_word(mine), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0ull;
    gu32* ep = (gu32*)(reinterpret_cast<unsigned*>(mine)) + b;
    const unsigned e = __hip_atomic_load(ep, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) + 1u;
    __hip_atomic_store(ep, e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    tag_s = e;
  }
  __syncthreads();
  if (failed_s) return;                                            // (uniform: no barrier skipped by some threads)
  const unsigned tag = tag_s;
  double st0 = 0.0, st1 = 0.0;                                     // (advanced at the end, as reduce_kernel)
  if (b == 0 && t == 0) { st0 = steps[0]; st1 = steps[1]; }
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
  bool ok = true;
  // 1: push this thread's float4 of each of the block's reduce_dp blocks to
  // the owners' reduce-scatter slot [rank]
  for (int rb = b; rb < nred; rb += nb) {
    const int64_t col = peer_col(L, g, H, rb, t);
    if (col >= 0) {
      const float4 v = reinterpret_cast<const float4*>(G)[col];
      const float e4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int64_t e = col * 4 + q, j = e / sl;
        peer_push(pb.buf[j], rs + (int64_t)rank * sl + (e - j * sl), tag, e4[q]);
      }
    }
  }
  // 2: this rank's slice, summed in rank order, / world, to every gather slot [rank]
  const int64_t mylen = min(sl, n - (int64_t)rank * sl);
  for (int64_t k = (int64_t)b * 256 + t; k < mylen; k += (int64_t)nb * 256) {
    float v = peer_pull(mine, rs + k, tag, mine, t0, ticks, ok);
    for (int j = 1; j < world; ++j) v += peer_pull(mine, rs + (int64_t)j * sl + k, tag, mine, t0, ticks, ok);
    v = v / (float)world;                                         // G.div_(world) (reduce_dp's IEEE division)
    // a sum with a missing term is never pushed: a slow peer must not take it
    // for a valid result (it times out, or fails fast on the error word)
    if (ok)
      for (int j = 0; j < world; ++j) peer_push(pb.buf[j], ag + (int64_t)rank * sl + k, tag, v);
  }
  // 3: gather each float4 into G; its squares to that reduce_dp block's norm pair
  for (int rb = b; rb < nred; rb += nb) {
    const int64_t col = peer_col(L, g, H, rb, t);
    double sa = 0.0, sc = 0.0;
    if (col >= 0) {
      float e4[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int64_t e = col * 4 + q, j = e / sl;
        e4[q] = peer_pull(mine, ag + j * sl + (e - j * sl), tag, mine, t0, ticks, ok);
      }
      const float4 v = make_float4(e4[0], e4[1], e4[2], e4[3]);
      reinterpret_cast<float4*>(G)[col] = v;
      const double q = sq4(v);
      const bool crit = net_of(L, col * 4, H);
      sa += crit ? 0.0 : q;
      sc += crit ? q : 0.0;
    }
    block_sum2(sa, sc, sh);
    if (t == 0) {
      nsq[2 * rb] = sa;
      nsq[2 * rb + 1] = sc;
    }
    __syncthreads();                                               // sh is reused by the next block_sum2
  }
  if (!ok) {
    // a peer never pushed (or one gave up): flag it in EVERY rank's buffer, so
    // a peer that is slow but alive fails this call too (its waits poll the
    // word) instead of completing it, and every later call returns at once
    for (int j = 0; j < world; ++j)
      __hip_atomic_store(peer_err_word(pb.buf[j]), 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  if (b == 0 && t == 0) { steps[0] = st0 + 1.0; steps[1] = st1 + 1.0; }
}


struct SpanLaunch { int kind; int64_t off, waves; };
struct SpanState {
  unsigned long long* buf = nullptr;
  int64_t words = 0, used = 0;
  std::vector<SpanLaunch> log;
};
SpanState g_span;

}  // namespace

unsigned long long* satrl_span::take(int kind, int64_t waves) {
  if (!g_span.buf || waves <= 0 || g_span.used + 2 * waves > g_span.words) return nullptr;
  unsigned long long* p = g_span.buf + g_span.used;
  g_span.log.push_back(SpanLaunch{kind, g_span.used, waves});
  g_span.used += 2 * waves;
  return p;
}

extern "C" {

int satrl_ppo_layout(int H, int64_t* off) {
  if (int rc = refuse(__func__, H, kAnyH, 1, "", 0, SATRL_PTRS(off))) return rc;
  const Layout L = layout(H);
  off[SATRL_PPO_OFF_W2] = L.W2;
  off[SATRL_PPO_OFF_W1] = L.W1;
  off[SATRL_PPO_OFF_B2] = L.b2;
  off[SATRL_PPO_OFF_W3A] = L.W3a;
  off[SATRL_PPO_OFF_B3A] = L.b3a;
  off[SATRL_PPO_OFF_LS] = L.ls;
  off[SATRL_PPO_OFF_W3C] = L.W3c;
  off[SATRL_PPO_OFF_B3C] = L.b3c;
  off[SATRL_PPO_TOTAL] = L.total;
  return 0;
}

// how the phases of the 32-row H 256 k-packed rowpass wait for each other
// (satrl_ppo_rowpass_sync): 0 workgroup barriers, 1 LDS hand-offs (RpHandoff).
// The hand-offs are the default: in-graph step at mb 4096 41.46-41.63 against
// 42.09-42.26 us over four alternations of 24 000 steps each, bench.py's
// update 39.32-39.43 against 40.24-40.33 us per step and its value +2.0-2.5 %
// in every pair; mb 512 (other kernels) unchanged (EXPERIMENTS.md, "Rowpass H 256:
// per-chunk LDS hand-offs")
#ifndef SATRL_RP_SYNC_DEFAULT
#define SATRL_RP_SYNC_DEFAULT 1
#endif
static std::atomic<int> g_rp_sync{SATRL_RP_SYNC_DEFAULT};
// whether a wave of that kernel (either sync form) may skip phase D
// (satrl_ppo_rowpass_dskip; rowpass_kernel, "D skip"): read at launch, passed
// as a kernel argument -- one instantiation serves both modes
#ifndef SATRL_RP_DSKIP_DEFAULT
#define SATRL_RP_DSKIP_DEFAULT 1
#endif
static std::atomic<int> g_rp_dskip{SATRL_RP_DSKIP_DEFAULT};

// ---------------------------------------------------------------------------
// The step plan (satrl_ppo_step_plan): which kernels step a minibatch and what
// their buffers hold, host arithmetic only.  launch_rowpass takes its kernel
// from rowpass_kind and the size queries of the ABI read plan_fill, so a
// threshold changes here and nowhere else.
// ---------------------------------------------------------------------------
// what a rowpass hands to dW2: f32 H1 / dZ2 rows, its own dW2 slabs (p2), or k-packed planes
enum RpOut { kRpOutRows, kRpOutDw2, kRpOutPlanes };
// row blocks by minibatch size, or 32-row blocks whatever the size (satrl_ppo_rowpass_kx32)
enum RpBlock { kRpBlockByMb, kRpBlock32 };

static int step_kind(int H) {
  return H == 64 ? SATRL_PPO_STEP_FUSED : H == 128 ? SATRL_PPO_STEP_ROWS : SATRL_PPO_STEP_KX;
}
static RpOut step_out(int step) {
  return step == SATRL_PPO_STEP_FUSED ? kRpOutDw2 : step == SATRL_PPO_STEP_KX ? kRpOutPlanes : kRpOutRows;
}
static int rp_rows(int kind) { return kind == SATRL_PPO_RP_WG16 || kind == SATRL_PPO_RP_CS ? kRowsShort : kRows; }
// the rowpass kernel (SATRL_PPO_RP_*) of one launch.  Only the k-packed H 256
// rowpass has more than the two block heights: the column split for both nets
// up to kCsMaxMb rows, the hand-off form of the 32-row kernel by the switch.
static int rowpass_kind(int H, int mb, int net, RpOut out, RpBlock block) {
  const int R = block == kRpBlock32 ? kRows : rows_per_wg(H, mb);
  if (H != 256 || out != kRpOutPlanes) return R == kRowsShort ? SATRL_PPO_RP_WG16 : SATRL_PPO_RP_WG32;
  if (R == kRowsShort) return net < 0 && mb <= kCsMaxMb ? SATRL_PPO_RP_CS : SATRL_PPO_RP_WG16;
  return g_rp_sync.load(std::memory_order_relaxed) == 1 ? SATRL_PPO_RP_WG32_HANDOFF : SATRL_PPO_RP_WG32;
}
// (H, mb, net checked by the caller)
static void plan_fill(int H, int mb, int net, satrl_ppo_plan* p) {
  const Layout L = layout(H);
  p->step = step_kind(H);
  p->rowpass = rowpass_kind(H, mb, net, step_out(p->step), kRpBlockByMb);
  p->rows_per_block = rp_rows(p->rowpass);
  p->row_blocks = n_head_wg(H, mb);
  p->error_word = p->rowpass == SATRL_PPO_RP_CS || p->rowpass == SATRL_PPO_RP_WG32_HANDOFF;
  p->slab_blocks = n_head_wg_cap(H, mb);                          // >= every minibatch of <= mb rows
  p->norm_blocks = n_blocks(geom(H, mb, 1, -1));                  // >= the per-net counts
  // splits of this minibatch, and their bound over every shorter one: a
  // shorter minibatch can split more ways (whole chunks, no empty split), but
  // never more ways than the workgroup target over the output tiles allows
  if (p->step == SATRL_PPO_STEP_FUSED) {                          // one slab per row block
    p->splits = p->row_blocks;
    p->max_splits = p->slab_blocks;
  } else if (p->step == SATRL_PPO_STEP_KX) {
    p->splits = kx_splits(mb, net);
    p->max_splits = std::max(p->splits, kKxWgs / kx_tiles(net));
  } else {                                                        // (both nets' count: a one-net call uses the same)
    p->splits = dw2_splits(H, mb, -1);
    p->max_splits = std::max(p->splits, kDwWgs / dw2_tiles(H, -1));
  }
  p->ptail_floats = p->slab_blocks * L.tail;
  p->pw1_floats = p->slab_blocks * 2 * H * 20;
  p->p2_floats = 2 * p->max_splits * H * H;
  p->kx_elems = p->step == SATRL_PPO_STEP_KX ? 2LL * 3 * kx_rows(mb) * H : 0;
  p->rows_floats = 2LL * mb * H;
}

// the checked plan: satrl_ppo_step_plan, and every size query that reads one field of it
static int plan_of(const char* who, int H, int widths, int mb, int net, satrl_ppo_plan* plan) {
  if (int rc = refuse(who, H, widths, mb, "mb", net, SATRL_PTRS(plan))) return rc;
  plan_fill(H, mb, net, plan);
  return 0;
}

int satrl_ppo_step_plan(int H, int mb, int net, satrl_ppo_plan* plan) {
  return plan_of(__func__, H, kAnyH, mb, net, plan);
}

int satrl_ppo_sizes(int H, int mb, int64_t* nwg, int64_t* nblk) {
  satrl_ppo_plan p;
  if (int rc = plan_of(__func__, H, kAnyH, mb, -1, &p)) return rc;
  if (nwg) *nwg = p.slab_blocks;
  if (nblk) *nblk = p.norm_blocks;
  return 0;
}

// the column-split short rowpass (rowpass_cs_kernel) runs when mb <= kCsMaxMb
// and every workgroup of its grid is resident at once (its groups wait on
// each other inside the launch): the occupancy API's answer, once per process
static bool cs_fits(int mb) {
  if (mb > kCsMaxMb) return false;
  static const int resident = [] {
    Residency r;
    return residency(rowpass_cs_kernel<false>, kCsWaves * 64, &r) ? r.blocks() : 0;
  }();
  return (2 * ((mb + kRowsShort - 1) / kRowsShort) + 7) / 8 * 32 <= resident;
}

// every rowpass entry point: `out` says what it writes for dW2 (kRpOutDw2, H <= 128:
// the block's dW2 partial to p2 instead of H1 / dZ2; kRpOutPlanes, H = 256: H1 /
// dZ2 are the k-packed planes) and with it which widths and outputs the call needs;
// `cap` is the caller's capacity of p2 or of the planes; ratio (nullable) receives
// the actor's per-row ratio
static int launch_rowpass(const char* who, int H, int mb, int net, const float* src, const int64_t* idx,
                          const float* P, const void* W2X, float epsilon, float ent_coef, float max_action, float* H1,
                          float* dZ2, float* ptail, float* pw1, float* p2, int64_t cap, float* ratio, RpOut out,
                          RpBlock block, void* stream) {
  const bool fdw2 = out == kRpOutDw2, kx = out == kRpOutPlanes;
  if (int rc = refuse(who, H, fdw2 ? kFusedH : kx ? 256 : kAnyH, mb, "mb", net, SATRL_PTRS(src, P, W2X, ptail, pw1)))
    return rc;
  // what it hands to dW2, and the caller's capacity for it (p2: one slab per row block)
  if (int rc = fdw2 ? null_arg(who, SATRL_PTRS(p2)) : null_arg(who, {kx ? "H1x, dZ2x" : "H1, dZ2", {H1, dZ2}}))
    return rc;
  if (int rc = fdw2 ? p2_fits(who, H, net, n_head_wg(H, mb), cap) : kx ? kx_fits(who, H, mb, net, cap) : 0) return rc;
  // the plan's kernel; the column split only when its grid is resident (else
  // the 16-wave kernel on the same 16-row blocks: the same bits)
  int kind = rowpass_kind(H, mb, net, out, block);
  if (kind == SATRL_PPO_RP_CS && !cs_fits(mb)) kind = SATRL_PPO_RP_WG16;
  const bool cs = kind == SATRL_PPO_RP_CS;
  const int R = rp_rows(kind), nrb = (mb + R - 1) / R;
  dim3 g((net < 0 ? 2 : 1) * nrb);   // (row block, net) pairs, or row blocks of one net
  const float inv_mb = 1.0f / (float)mb;
  // waves per workgroup: one 16-column tile per wave for both 16-row tiles
  const int nw = waves_of<kNW256>(H);
  // (the column-split kernel: groups of kCsSplit workgroups dealt in windows of 32 blocks)
  const dim3 gc((unsigned)((2 * nrb + 7) / 8 * 32));
  unsigned long long* sp =
      satrl_span::take(satrl_span::kRowpass, cs ? (int64_t)gc.x * kCsWaves : (int64_t)g.x * nw);
  auto rp = [&](auto k) {
    launch_span(k.first, k.second, sp, g, dim3(nw * 64), stream, mb, net, src, idx, P, W2X, H1, dZ2, epsilon,
                ent_coef, max_action, ptail, pw1, p2, nrb, ratio, inv_mb, g_rp_dskip.load(std::memory_order_relaxed));
  };
  with_width<kNW256>(H, [&](auto w) {
    using W = decltype(w);
    if constexpr (W::H != 256)
      fdw2 ? rp(rowpass_k<W::H, W::NW, kRows, true, false>()) : rp(rowpass_k<W::H, W::NW, kRows, false, false>());
    else if (cs)
      launch_span(rowpass_cs_kernel<true>, rowpass_cs_kernel<false>, sp, gc, dim3(kCsWaves * 64), stream, mb, src, idx,
                  P, static_cast<const float*>(W2X), epsilon, ent_coef, max_action,
                  reinterpret_cast<unsigned short*>(H1), reinterpret_cast<unsigned short*>(dZ2), ptail, pw1, inv_mb);
    else if (kind == SATRL_PPO_RP_WG16)
      kx ? rp(rowpass_k<256, W::NW, kRowsShort, false, true>()) : rp(rowpass_k<256, W::NW, kRowsShort, false, false>());
    else if (kind == SATRL_PPO_RP_WG32_HANDOFF)
      rp(rowpass_k<256, W::NW, kRows, false, true, true>());
    else
      kx ? rp(rowpass_k<256, W::NW, kRows, false, true>()) : rp(rowpass_k<256, W::NW, kRows, false, false>());
  });
  return launched(who);
}

int satrl_ppo_rowpass(int H, int mb, int net, const float* src, const int64_t* idx, const float* P, const void* W2X,
                      float epsilon, float ent_coef, float max_action, float* H1, float* dZ2, float* ptail,
                      float* pw1, void* stream) {
  return launch_rowpass(__func__, H, mb, net, src, idx, P, W2X, epsilon, ent_coef, max_action, H1, dZ2,
                        ptail, pw1, nullptr, 0, nullptr, kRpOutRows, kRpBlockByMb, stream);
}

int satrl_ppo_rowpass_ratio(int H, int mb, int net, const float* src, const int64_t* idx, const float* P,
                            const void* W2X, float epsilon, float ent_coef, float max_action, float* H1, float* dZ2,
                            float* ptail, float* pw1, float* ratio, void* stream) {
  if (!ratio) return fail(-1, __func__, "ratio is NULL");
  return launch_rowpass(__func__, H, mb, net, src, idx, P, W2X, epsilon, ent_coef, max_action, H1,
                        dZ2, ptail, pw1, nullptr, 0, ratio, kRpOutRows, kRpBlockByMb, stream);
}

int satrl_ppo_row_blocks(int H, int mb) {
  satrl_ppo_plan p;
  return plan_of(__func__, H, kAnyH, mb, -1, &p) ? -1 : p.row_blocks;
}

int satrl_ppo_rowpass_dw2(int H, int mb, int net, const float* src, const int64_t* idx, const float* P,
                          const void* W2X, float epsilon, float ent_coef, float max_action, float* p2,
                          int64_t p2_floats, float* ptail, float* pw1, void* stream) {
  return launch_rowpass(__func__, H, mb, net, src, idx, P, W2X, epsilon, ent_coef, max_action, nullptr,
                        nullptr, ptail, pw1, p2, p2_floats, nullptr, kRpOutDw2, kRpBlockByMb, stream);
}

int64_t satrl_ppo_kx_elems(int H, int mb) {
  satrl_ppo_plan p;
  return plan_of(__func__, H, 256, mb, -1, &p) ? -1 : p.kx_elems;
}

int satrl_ppo_rowpass_kx(int H, int mb, int net, const float* src, const int64_t* idx, const float* P, const void* W2X,
                         float epsilon, float ent_coef, float max_action, void* H1x, void* dZ2x, int64_t kx_elems,
                         float* ptail, float* pw1, void* stream) {
  return launch_rowpass(__func__, H, mb, net, src, idx, P, W2X, epsilon, ent_coef, max_action,
                        static_cast<float*>(H1x), static_cast<float*>(dZ2x), ptail, pw1, nullptr, kx_elems, nullptr,
                        kRpOutPlanes, kRpBlockByMb, stream);
}

int satrl_ppo_rowpass_kx32(int H, int mb, int net, const float* src, const int64_t* idx, const float* P,
                           const void* W2X, float epsilon, float ent_coef, float max_action, void* H1x, void* dZ2x,
                           int64_t kx_elems, float* ptail, float* pw1, float* ratio, void* stream) {
  return launch_rowpass(__func__, H, mb, net, src, idx, P, W2X, epsilon, ent_coef, max_action,
                        static_cast<float*>(H1x), static_cast<float*>(dZ2x), ptail, pw1, nullptr, kx_elems, ratio,
                        kRpOutPlanes, kRpBlock32, stream);
}

int satrl_ppo_rowpass_sync(int mode) {
  if (int rc = outside(__func__, "mode", mode, -1, 1)) return rc;
  return mode < 0 ? g_rp_sync.load(std::memory_order_relaxed) : g_rp_sync.exchange(mode, std::memory_order_relaxed);
}

int satrl_ppo_rowpass_dskip(int mode) {
  if (int rc = outside(__func__, "mode", mode, -1, 1)) return rc;
  return mode < 0 ? g_rp_dskip.load(std::memory_order_relaxed) : g_rp_dskip.exchange(mode, std::memory_order_relaxed);
}

int satrl_ppo_rowpass_error(int* err, double timeout_s, void* stream) {
  if (int rc = null_arg(__func__, SATRL_PTRS(err))) return rc;
  if (!(timeout_s > 0)) return fail(-1, __func__, "timeout_s is not positive: no deadline");
  hipStream_t s = (hipStream_t)stream;
  // the error word lands in pinned memory behind an event that is polled
  // against the host deadline: a stream that never drains (e.g. a collective
  // of a dead peer queued before this call) returns -2 instead of hanging.
  // After a timeout the buffer and event stay with the stream (leaked): the
  // next call takes fresh ones.
  static std::mutex mu;
  static unsigned* host = nullptr;
  static hipEvent_t ev = nullptr;
  std::lock_guard<std::mutex> lock(mu);
  void *pe = nullptr, *pc = nullptr;
  if ((!host && hipHostMalloc((void**)&host, 4 * sizeof(unsigned), hipHostMallocDefault) != hipSuccess) ||
      (!ev && hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) ||
      hipGetSymbolAddress(&pe, HIP_SYMBOL(g_cs_err)) != hipSuccess ||
      hipGetSymbolAddress(&pc, HIP_SYMBOL(g_cs_ctr)) != hipSuccess ||
      hipMemcpyAsync(host, pe, sizeof(unsigned), hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipEventRecord(ev, s) != hipSuccess)
    return fail(-1, __func__, "reading the exchange error word failed");
  const auto t0 = std::chrono::steady_clock::now();
  for (;;) {
    const hipError_t q = hipEventQuery(ev);
    if (q == hipSuccess) break;
    if (q != hipErrorNotReady) return fail(-1, __func__, "waiting for the stream failed");
    if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > timeout_s) {
      host = nullptr;
      ev = nullptr;
      return fail(-2, __func__, "the stream did not drain within the deadline");
    }
    std::this_thread::sleep_for(std::chrono::microseconds(20));
  }
  const unsigned e = host[0];
  *err = e != 0;
  if (e != 0 && (hipMemsetAsync(pe, 0, sizeof(g_cs_err), s) != hipSuccess ||
                 hipMemsetAsync(pc, 0, sizeof(g_cs_ctr), s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess))
    return fail(-1, __func__, "re-arming the exchange state failed");
  return 0;
}

int satrl_ppo_rowpass_fault_inject(int group, unsigned value, void* stream) {
  if (int rc = outside(__func__, "group", group, 0, kCsMaxGroups - 1)) return rc;
  hipStream_t s = (hipStream_t)stream;
  void* pc = nullptr;
  if (hipGetSymbolAddress(&pc, HIP_SYMBOL(g_cs_ctr)) != hipSuccess ||
      hipMemcpyAsync(static_cast<unsigned*>(pc) + (size_t)group * 32, &value, sizeof(value), hipMemcpyHostToDevice, s) !=
          hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return fail(-1, __func__, "writing the exchange counter failed");
  return 0;
}

int satrl_ppo_dw2_kx_splits(int H, int mb, int net) {
  satrl_ppo_plan p;
  return plan_of(__func__, H, 256, mb, net, &p) ? -1 : p.splits;
}

// what both k-packed dW2 entry points refuse; *kr: the rows of one split
static int dw2_kx_check(const char* who, int H, int mb, int net, int S, const void* H1x, const void* dZ2x,
                        int64_t kx_elems, float* p2, int64_t p2_floats, int* kr) {
  if (int rc = refuse(who, H, 256, mb, "mb", net, SATRL_PTRS(H1x, dZ2x, p2))) return rc;
  if (int rc = split_size(who, S, (int)kx_rows(mb), 32, "satrl_ppo_dw2_kx_splits", kr)) return rc;   // whole chunks
  if (int rc = kx_fits(who, H, mb, net, kx_elems)) return rc;
  return p2_fits(who, H, net, S, p2_floats);
}

int satrl_ppo_dw2_kx(int H, int mb, int net, int S, const void* H1x, const void* dZ2x, int64_t kx_elems, float* p2,
                     int64_t p2_floats, void* stream) {
  int kr = 0;
  if (int rc = dw2_kx_check(__func__, H, mb, net, S, H1x, dZ2x, kx_elems, p2, p2_floats, &kr)) return rc;
  const dim3 g((unsigned)(kx_tiles(net) * S));
  unsigned long long* sp = satrl_span::take(satrl_span::kDw2, (int64_t)g.x * 4);
  launch_span(dw2_kx_kernel<kKxTW, true>, dw2_kx_kernel<kKxTW>, sp, g, dim3(256), stream, mb, S, kr, net,
              static_cast<const unsigned short*>(H1x), static_cast<const unsigned short*>(dZ2x), p2);
  return launched(__func__);
}

int satrl_ppo_dw2_kx_w1(int H, int mb, int net, int S, const void* H1x, const void* dZ2x, int64_t kx_elems, float* p2,
                        int64_t p2_floats, int mode, const float* p1, const float* pt, float* G, double* nsq,
                        void* stream) {
  int kr = 0;
  if (int rc = dw2_kx_check(__func__, H, mb, net, S, H1x, dZ2x, kx_elems, p2, p2_floats, &kr)) return rc;
  if (mode != 1 && mode != 3) return fail(-1, __func__, "mode " + to_string(mode) + " is not 1 or 3");
  if (int rc = null_arg(__func__, SATRL_PTRS(p1, pt, G))) return rc;
  if ((mode & 2) && !nsq) return fail(-1, __func__, "nsq is NULL with mode 3");
  const RedGeom rg = geom(H, mb, S, net);
  const int ndw = kx_tiles(net) * S;
  const dim3 g((unsigned)(ndw + rg.nb1 + rg.nbt));
  unsigned long long* sp = satrl_span::take(satrl_span::kDw2, (int64_t)g.x * 4);
  const unsigned short *h1 = static_cast<const unsigned short*>(H1x), *dz = static_cast<const unsigned short*>(dZ2x);
  launch_span(dw2_kx_w1_kernel<kKxTW, true>, dw2_kx_w1_kernel<kKxTW>, sp, g, dim3(256), stream, mb, S, kr, net, h1, dz,
              p2, ndw, rg, mode, p1, pt, G, nsq);
  return launched(__func__);
}

int satrl_ppo_dw2_splits(int H, int mb) {
  return refuse(__func__, H, kAnyH, mb, "mb", -1) ? -1 : dw2_splits(H, mb, -1);
}

int satrl_ppo_dw2(int H, int mb, int net, int S, const float* H1, const float* dZ2, float* p2, int64_t p2_floats,
                  void* stream) {
  if (int rc = refuse(__func__, H, kAnyH, mb, "mb", net, SATRL_PTRS(H1, dZ2, p2))) return rc;
  int KR = 0;
  if (int rc = split_size(__func__, S, mb, kDwKC, "satrl_ppo_dw2_splits", &KR)) return rc;
  if (int rc = p2_fits(__func__, H, net, S, p2_floats)) return rc;
  const char* who = __func__;
  return with_width<kNW256>(H, [&](auto w) {                      // (dw2_kernel takes the width alone)
    return launch(who, dw2_kernel<decltype(w)::H>, dw2_tiles(H, net) * S, 256, stream, mb, S, KR, net, H1, dZ2, p2);
  });
}

int satrl_ppo_reduce(int H, int mb, int net, int S, int mode, const float* p2, int64_t p2_floats, const float* p1,
                     const float* pt, float* G, double* nsq, double* steps, void* stream) {
  // mode bit 4: the W2 region only (satrl_ppo_dw2_kx_w1 summed the others)
  const bool w2_only = (mode & 4) != 0;
  mode &= 3;
  if (int rc = refuse(__func__, H, kAnyH, mb, "mb", net, SATRL_PTRS(G))) return rc;
  if (S < 1) return fail(-1, __func__, "S " + to_string(S) + " < 1");
  if (mode < 1 || (w2_only && !(mode & 1))) return fail(-1, __func__, "mode has no bit 1 or 2, or bit 4 without 1");
  if (mode & 1) {
    if (int rc = w2_only ? null_arg(__func__, SATRL_PTRS(p2)) : null_arg(__func__, SATRL_PTRS(p2, p1, pt))) return rc;
    if (int rc = p2_fits(__func__, H, net, S, p2_floats)) return rc;   // the slabs it reads
  }
  if (mode & 2)
    if (int rc = null_arg(__func__, SATRL_PTRS(nsq, steps))) return rc;
  const RedGeom g = geom(H, mb, S, net);
  const int nb = w2_only ? g.nb2 : n_blocks(g);
  unsigned long long* sp = satrl_span::take(satrl_span::kReduce, (int64_t)nb * 4);
  launch_span(reduce_kernel<true>, reduce_kernel<false>, sp, dim3(nb), dim3(256), stream, H, mode, g.nb2, g.S,
              g.net, g.ch2, p2, steps, G, nsq, g, p1, pt, 1);
  return launched(__func__);
}

int satrl_ppo_reduce_dp(int H, int mb, int net, int world, float* G, double* nsq, double* steps, void* stream) {
  if (int rc = refuse(__func__, H, kAnyH, mb, "mb", net, SATRL_PTRS(G, nsq, steps))) return rc;
  if (world < 1) return fail(-1, __func__, "world " + to_string(world) + " < 1");
  const RedGeom g = geom(H, mb, 1, net);
  return launch(__func__, reduce_kernel<false>, n_blocks(g), 256, stream, H, 2, g.nb2, g.S, g.net, g.ch2, nullptr,
                steps, G, nsq, g, nullptr, nullptr, world, nullptr);
}

// a failed HIP call of `who` (not a launch): -2 with what was attempted and HIP's text
static int hip_failed(const char* who, const char* what) {
  return fail(-2, who, std::string(what) + " failed: " + hipGetErrorString(hipGetLastError()));
}

int satrl_peer_buffer_bytes(int64_t n, int world, int64_t* bytes) {
  if (n <= 0) return fail(-1, __func__, "n " + to_string(n) + " <= 0");
  if (int rc = outside(__func__, "world", world, 1, kPeerMaxW)) return rc;
  if (int rc = null_arg(__func__, SATRL_PTRS(bytes))) return rc;
  *bytes = peer_bytes(n, world);
  return 0;
}

int satrl_peer_alloc(int64_t bytes, void** buf, void* ipc_handle) {
  if (bytes <= 0) return fail(-1, __func__, "bytes " + to_string(bytes) + " <= 0");
  if (int rc = null_arg(__func__, SATRL_PTRS(buf, ipc_handle))) return rc;
  void* p = nullptr;
  if (hipExtMallocWithFlags(&p, (size_t)bytes, hipDeviceMallocUncached) != hipSuccess)
    return hip_failed(__func__, "hipExtMallocWithFlags(uncached)");
  hipIpcMemHandle_t h;
  if (hipMemset(p, 0, (size_t)bytes) != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
      hipIpcGetMemHandle(&h, p) != hipSuccess) {
    const int rc = hip_failed(__func__, "zeroing / hipIpcGetMemHandle");
    (void)hipFree(p);
    return rc;
  }
  std::memcpy(ipc_handle, &h, sizeof(h));
  *buf = p;
  return 0;
}

int satrl_peer_open(const void* ipc_handle, void** buf) {
  if (int rc = null_arg(__func__, SATRL_PTRS(ipc_handle, buf))) return rc;
  hipIpcMemHandle_t h;
  std::memcpy(&h, ipc_handle, sizeof(h));
  if (hipIpcOpenMemHandle(buf, h, hipIpcMemLazyEnablePeerAccess) != hipSuccess)
    return hip_failed(__func__, "hipIpcOpenMemHandle");
  return 0;
}

int satrl_peer_close(void* buf) {
  if (!buf) return fail(-2, __func__, "buf is NULL");
  return hipIpcCloseMemHandle(buf) == hipSuccess ? 0 : hip_failed(__func__, "hipIpcCloseMemHandle");
}
int satrl_peer_free(void* buf) {
  if (!buf) return fail(-2, __func__, "buf is NULL");
  return hipFree(buf) == hipSuccess ? 0 : hip_failed(__func__, "hipFree");
}

int satrl_peer_error(const void* buf, uint64_t* err, void* stream) {
  if (int rc = null_arg(__func__, SATRL_PTRS(buf, err))) return rc;
  hipStream_t st = (hipStream_t)stream;               // ordered after the calls queued on `stream`
  const char* word = static_cast<const char*>(buf) + 4 * kPeerMaxBlocks;
  if (hipMemcpyAsync(err, word, 8, hipMemcpyDeviceToHost, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess)
    return 0;
  return hip_failed(__func__, "reading the error word");
}

int satrl_peer_reset(void* buf, int64_t bytes, void* stream) {
  if (int rc = null_arg(__func__, SATRL_PTRS(buf))) return rc;
  if (bytes < kPeerHdr)
    return fail(-1, __func__, to_string(bytes) + " bytes are smaller than the header, " + to_string(kPeerHdr));
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(buf, 0, (size_t)bytes, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess) return 0;
  return hip_failed(__func__, "zeroing the buffer");
}

// the peer kernel's grid at width H: reduce_dp's block count, capped at one
// block per CU of the current device and at what can be resident at once
int satrl_peer_blocks(int H, int* blocks) {
  if (int rc = refuse(__func__, H, kAnyH, 1, "", 0, SATRL_PTRS(blocks))) return rc;
  Residency r;
  if (!residency(peer_allreduce_kernel, 256, &r)) return hip_failed(__func__, "the device query");
  *blocks = std::min(n_blocks(geom(H, 1, 1, -1)), std::min(r.cus, r.blocks()));
  return *blocks > 0 ? 0 : fail(-2, __func__, "no block of the peer kernel can be resident");
}

int satrl_ppo_allreduce_peer(int H, int mb, int world, int rank, void* const* bufs, float* G, double* nsq,
                             double* steps, int blocks, double timeout_s, void* stream) {
  if (int rc = refuse(__func__, H, kAnyH, mb, "mb", 0)) return rc;
  if (int rc = outside(__func__, "world", world, 1, kPeerMaxW)) return rc;
  if (int rc = outside(__func__, "rank", rank, 0, world - 1)) return rc;
  if (int rc = null_arg(__func__, SATRL_PTRS(bufs, G, nsq, steps))) return rc;
  if (int rc = outside(__func__, "blocks", blocks, 1, kPeerMaxBlocks)) return rc;
  if (!(timeout_s > 0.0) || timeout_s > 1e7) return fail(-1, __func__, "timeout_s is not in (0, 1e7]: no deadline");
  PeerBufs pb{};
  for (int j = 0; j < world; ++j) {
    if (!bufs[j]) return fail(-1, __func__, "bufs[" + to_string(j) + "] is NULL");
    pb.buf[j] = static_cast<unsigned long long*>(bufs[j]);
  }
  // every block must be resident at once (a block waits on values other blocks push)
  Residency r;
  if (!residency(peer_allreduce_kernel, 256, &r)) return hip_failed(__func__, "the device query");
  if (blocks > r.blocks())
    return fail(-1, __func__, to_string(blocks) + " blocks cannot all be resident (" + to_string(r.cus) +
                             " CUs x " + to_string(r.per_cu) + ")");
  const RedGeom g = geom(H, mb, 1, -1);
  const unsigned long long ticks = (unsigned long long)(timeout_s * 1e8);   // s_memrealtime: 100 MHz
  return launch(__func__, peer_allreduce_kernel, blocks, 256, stream, H, g, world, rank, pb, G, nsq, steps, ticks);
}

int satrl_ppo_adam(int H, int mb, int net, const double* nsq, const double* steps, const double* bct, int bct_len,
                   const float* lr, float beta1, float beta2, float eps, float max_norm, int use_clip, const float* G,
                   float* P, float* M, float* V, void* W2X, void* stream) {
  if (int rc = refuse(__func__, H, kAnyH, mb, "mb", net, SATRL_PTRS(nsq, steps, bct, lr, G, P, M, V))) return rc;
  if (bct_len < 1) return fail(-1, __func__, "bct_len " + to_string(bct_len) + " < 1");
  const int nblk = n_blocks(geom(H, mb, 1, net));
  unsigned long long* sp = satrl_span::take(satrl_span::kAdam, (int64_t)n_adam_blocks(H, net) * 4);
  launch_span(adam_kernel<true>, adam_kernel<false>, sp, dim3(n_adam_blocks(H, net)), dim3(256), stream, H, nblk, nsq,
              G, P, M, V, net, bct_len, steps, bct, lr, beta1, beta2, eps, max_norm, use_clip, W2X);
  return launched(__func__);
}

int64_t satrl_ppo_w2x_floats(int H) {
  return refuse(__func__, H, kAnyH, 1, "", 0) ? -1 : w2x_floats(H);
}

int satrl_ppo_w2x_sync(int H, int net, const float* P, void* W2X, void* stream) {
  if (int rc = refuse(__func__, H, kAnyH, 1, "", net, SATRL_PTRS(P, W2X))) return rc;
  const int ntc = H / 32;
  return launch(__func__, w2x_sync_kernel, (net < 0 ? 2 : 1) * ntc * ntc, 256, stream, H, net, P, W2X);
}

int satrl_ppo_stage(int64_t rows, const float* src, const int64_t* perm, const int64_t* group, float* stage,
                    void* stream) {
  if (rows <= 0) return fail(-1, __func__, "rows " + to_string(rows) + " <= 0");
  if (int rc = null_arg(__func__, SATRL_PTRS(src, perm, group, stage))) return rc;
  return launch(__func__, stage_kernel, (rows * 8 + 255) / 256, 256, stream, rows,
                reinterpret_cast<const float4*>(src), perm, group, reinterpret_cast<float4*>(stage));
}

int satrl_ppo_group_advance(int64_t* group, void* stream) {
  if (int rc = null_arg(__func__, SATRL_PTRS(group))) return rc;
  return launch(__func__, group_advance_kernel, 1, 1, stream, group);
}

int satrl_policy_act(int H, int64_t N, const float* obs, const float* P0, const float* P1, float max_action,
                     uint64_t seed, int64_t env_offset, uint64_t step, const uint64_t* step_base, float* act0,
                     float* logp0, float* act1, float* logp1, void* stream) {
  if (int rc = refuse(__func__, H, kAnyH, N, "N", 0, SATRL_PTRS(obs, P0, act0, logp0))) return rc;
  if (P1)                                                          // a second agent brings its outputs
    if (int rc = null_arg(__func__, SATRL_PTRS(act1, logp1))) return rc;
  const int nag = P1 ? 2 : 1;
  const PolicyKeys k(seed);
  return launch_policy<0>(__func__, H, satrl_span::kPolicyAct, nag, N, stream, obs, P0, P1, nag, max_action, k.k00,
                          k.k01, k.k10, k.k11, env_offset, step, step_base, act0, logp0, act1, logp1, nullptr, 0);
}

int satrl_policy_act_pool(int H, int64_t N, const float* obs, const float* P0, const float* P1, float max_action,
                          uint64_t seed, int64_t env_offset, uint64_t step, const uint64_t* step_base, float* act0,
                          float* logp0, float* act1, float* logp1, int pool_agent, const float* pool,
                          int64_t pool_stride, int K, const int32_t* member, void* stream) {
  if (int rc = refuse(__func__, H, kAnyH, N, "N", 0, SATRL_PTRS(obs, P0, act0, logp0))) return rc;
  if (!P1 || !act1 || !logp1) return fail(-1, __func__, "both agents are required: a NULL P1, act1 or logp1");
  if (pool_agent != 0 && pool_agent != 1) return fail(-1, __func__, "pool_agent is 0 or 1");
  if (int rc = null_arg(__func__, SATRL_PTRS(pool, member))) return rc;
  if (K <= 0) return fail(-1, __func__, "K <= 0");
  if (pool_stride < layout(H).total || pool_stride % 4 != 0)
    return fail(-1, __func__, "pool_stride below the layout total or not a multiple of 4");
  if (reinterpret_cast<uintptr_t>(pool) & 15) return fail(-1, __func__, "pool is not 16-byte aligned");
  const PolicyKeys k(seed);
  const char* who = __func__;
  // (no SPAN form: under a span probe this is the launch, and nothing is logged)
  return with_width<kPolNW>(H, [&](auto w) {
    using W = decltype(w);
    return launch(who, policy_pool_kernel<W::H, W::NW>, 2 * ((N + kPolRows - 1) / kPolRows), W::NW * 64, stream, N, obs,
                  pool, member, pool_stride, K, pool_agent, P0, P1, max_action, k.k00, k.k01, k.k10, k.k11, env_offset,
                  step, step_base, act0, logp0, act1, logp1);
  });
}

int satrl_opponent_assign(uint64_t seed, uint64_t iteration, int64_t first_block, int64_t n_blocks, int filled,
                          double latest_prob, int32_t* member_out) {
  if (!member_out || n_blocks <= 0 || first_block < 0 || filled < 0 || !(latest_prob >= 0.0 && latest_prob <= 1.0))
    return fail(-1, __func__,
                "a NULL output, n_blocks <= 0, first_block < 0, filled < 0, or latest_prob outside [0, 1]");
  uint32_t k0, k1;
  philox_key(seed, 3, k0, k1);
  for (int64_t i = 0; i < n_blocks; ++i) {
    const uint64_t g = (uint64_t)first_block + (uint64_t)i;
    uint32_t w[4] = {(uint32_t)g, (uint32_t)(g >> 32), (uint32_t)iteration, (uint32_t)(iteration >> 32)};
    philox4x32_10(w, k0, k1);
    const double u = ((double)w[0] + 0.5) * (1.0 / 4294967296.0);
    member_out[i] = (filled == 0 || u < latest_prob) ? -1 : (int32_t)(((uint64_t)w[1] * (uint64_t)filled) >> 32);
  }
  return 0;
}

int satrl_policy_act_league(int H, int64_t N, const float* obs, const float* P0, const float* P1, float max_action,
                            uint64_t seed, int64_t env_offset, uint64_t step, const uint64_t* step_base, float* act0,
                            float* logp0, float* act1, float* logp1, int pool_agent, const float* pool,
                            int64_t pool_stride, int K, const int32_t* member, const float* obs_law,
                            const satrl_scripted_law* laws, int J, void* stream) {
  if (int rc = refuse(__func__, H, kAnyH, N, "N", 0, SATRL_PTRS(obs, P0, act0, logp0))) return rc;
  if (!P1 || !act1 || !logp1) return fail(-1, __func__, "both agents are required: a NULL P1, act1 or logp1");
  if (pool_agent != 0 && pool_agent != 1) return fail(-1, __func__, "pool_agent is 0 or 1");
  if (int rc = null_arg(__func__, SATRL_PTRS(pool, member, obs_law, laws))) return rc;
  if (K <= 0) return fail(-1, __func__, "K <= 0");
  if (pool_stride < layout(H).total || pool_stride % 4 != 0)
    return fail(-1, __func__, "pool_stride below the layout total or not a multiple of 4");
  if (reinterpret_cast<uintptr_t>(pool) & 15) return fail(-1, __func__, "pool is not 16-byte aligned");
  if (J < 1 || J > SATRL_LEAGUE_MAX_LAWS)
    return fail(-1, __func__, "J " + to_string(J) + " is outside 1 .. " + to_string(SATRL_LEAGUE_MAX_LAWS));
  if (reinterpret_cast<uintptr_t>(laws) & 7) return fail(-1, __func__, "laws is not 8-byte aligned");
  const PolicyKeys k(seed);
  const char* who = __func__;
  // (no SPAN form, as satrl_policy_act_pool)
  return with_width<kPolNW>(H, [&](auto w) {
    using W = decltype(w);
    return launch(who, policy_league_kernel<W::H, W::NW>, 2 * ((N + kPolRows - 1) / kPolRows), W::NW * 64, stream, N,
                  obs, pool, member, pool_stride, K, pool_agent, J, max_action, P0, P1, obs_law, laws, k.k00, k.k01,
                  k.k10, k.k11, env_offset, step, step_base, act0, logp0, act1, logp1);
  });
}

int satrl_league_assign(uint64_t seed, uint64_t iteration, int64_t first_block, int64_t n_blocks, int K, int filled,
                        int n_laws, double latest_prob, double law_prob, const double* weights,
                        int32_t* member_out) {
  if (!member_out) return fail(-1, __func__, "member_out is NULL");
  if (n_blocks <= 0) return fail(-1, __func__, "n_blocks " + to_string(n_blocks) + " <= 0");
  if (first_block < 0) return fail(-1, __func__, "first_block " + to_string(first_block) + " < 0");
  if (K < 0) return fail(-1, __func__, "K " + to_string(K) + " < 0");
  if (filled < 0 || filled > K)
    return fail(-1, __func__, "filled " + to_string(filled) + " is outside 0 .. K = " + to_string(K));
  if (n_laws < 0 || n_laws > SATRL_LEAGUE_MAX_LAWS)
    return fail(-1, __func__, "n_laws " + to_string(n_laws) + " is outside 0 .. " + to_string(SATRL_LEAGUE_MAX_LAWS));
  if (!(latest_prob >= 0.0 && latest_prob <= 1.0)) return fail(-1, __func__, "latest_prob is outside [0, 1]");
  if (!(law_prob >= 0.0 && law_prob <= 1.0)) return fail(-1, __func__, "law_prob is outside [0, 1]");
  const double law_edge = latest_prob + law_prob;
  if (!(law_edge <= 1.0)) return fail(-1, __func__, "latest_prob + law_prob is above 1");
  double S = 0.0;
  int last_pos = -1;
  if (weights && filled > 0) {
    for (int k = 0; k < filled; ++k) {
      if (!(weights[k] >= 0.0) || !std::isfinite(weights[k]))
        return fail(-1, __func__, "weights[" + to_string(k) + "] is negative or not finite");
      S += weights[k];
      if (weights[k] > 0.0) last_pos = k;
    }
    if (!(S > 0.0) || !std::isfinite(S)) return fail(-1, __func__, "the sum of weights is not positive and finite");
  }
  uint32_t k0, k1;
  philox_key(seed, 3, k0, k1);
  for (int64_t i = 0; i < n_blocks; ++i) {
    const uint64_t g = (uint64_t)first_block + (uint64_t)i;
    uint32_t w[4] = {(uint32_t)g, (uint32_t)(g >> 32), (uint32_t)iteration, (uint32_t)(iteration >> 32)};
    philox4x32_10(w, k0, k1);
    const double u = ((double)w[0] + 0.5) * (1.0 / 4294967296.0);
    int32_t m;
    if ((filled == 0 && n_laws == 0) || u < latest_prob) {
      m = -1;
    } else if (n_laws > 0 && (filled == 0 || u < law_edge)) {
      m = K + (int32_t)(((uint64_t)w[2] * (uint64_t)n_laws) >> 32);
    } else if (!weights) {
      m = (int32_t)(((uint64_t)w[1] * (uint64_t)filled) >> 32);
    } else {
      const double v = ((double)w[1] + 0.5) * (1.0 / 4294967296.0) * S;
      double c = 0.0;
      m = last_pos;
      for (int k = 0; k < filled; ++k) {
        c += weights[k];
        if (v < c) {
          m = k;
          break;
        }
      }
    }
    member_out[i] = m;
  }
  return 0;
}

int satrl_policy_eval(int H, int64_t N, const float* obs, const float* P0, const float* P1, float max_action,
                      int det_mask, uint64_t seed, int64_t env_offset, uint64_t step, const uint64_t* step_base,
                      float* act0, float* act1, void* stream) {
  if (int rc = refuse(__func__, H, kAnyH, N, "N", 0, SATRL_PTRS(obs, P0, act0))) return rc;
  if (det_mask < 0 || det_mask > 3 || ((det_mask & 2) && !P1))
    return fail(-1, __func__, "det_mask " + to_string(det_mask) + " is outside 0 .. 3, or has bit 2 without P1");
  if (P1 && !act1) return fail(-1, __func__, "act1 is NULL");
  const int nag = P1 ? 2 : 1;
  const PolicyKeys k(seed);
  return launch_policy<2>(__func__, H, satrl_span::kPolicyAct, nag, N, stream, obs, P0, P1, nag, max_action, k.k00,
                          k.k01, k.k10, k.k11, env_offset, step, step_base, act0, nullptr, act1, nullptr, nullptr,
                          det_mask);
}

int satrl_scripted_act(int64_t N, const float* obs, const satrl_scripted_law* law, float* act, void* stream) {
  if (N <= 0) return fail(-1, __func__, "N " + to_string(N) + " <= 0");
  if (int rc = null_arg(__func__, SATRL_PTRS(obs, law, act))) return rc;
  return launch(__func__, scripted_kernel, (N + kScriptedBlock - 1) / kScriptedBlock, kScriptedBlock, stream, N, obs,
                law, act);
}

int satrl_policy_act_scripted(int H, int64_t N, const float* obs, const float* obs_law, const float* P, int agent,
                              float max_action, uint64_t seed, int64_t env_offset, uint64_t step,
                              const uint64_t* step_base, float* act, float* logp, const satrl_scripted_law* law,
                              float* act_scripted, void* stream) {
  return launch_policy_scripted<0>(__func__, H, N, obs, obs_law, P, agent, max_action, 0, seed,
                                   env_offset, step, step_base, act, logp, law, act_scripted, stream);
}

int satrl_policy_eval_scripted(int H, int64_t N, const float* obs, const float* obs_law, const float* P, int agent,
                               float max_action, int det, uint64_t seed, int64_t env_offset, uint64_t step,
                               const uint64_t* step_base, float* act, const satrl_scripted_law* law,
                               float* act_scripted, void* stream) {
  return launch_policy_scripted<2>(__func__, H, N, obs, obs_law, P, agent, max_action, det, seed,
                                   env_offset, step, step_base, act, nullptr, law, act_scripted, stream);
}

int satrl_policy_value(int H, int64_t N, const float* obs, const float* P, float* v_out, void* stream) {
  if (int rc = refuse(__func__, H, kAnyH, N, "N", 0, SATRL_PTRS(obs, P, v_out))) return rc;
  return launch_policy<1>(__func__, H, satrl_span::kPolicyValue, 1, N, stream, obs, P, nullptr, 1, 0.0f, 0u, 0u, 0u, 0u,
                          (int64_t)0, (uint64_t)0, nullptr, nullptr, nullptr, nullptr, nullptr, v_out, 0);
}

// f64 elements of satrl_ppo_diagnostics' scratch: a line per 32-row block, and
// above kDiagChunk blocks a line per chunk of them (the first reduce level)
static int64_t diag_scratch(const char* who, int64_t n) {
  if (n <= 0 || n > (int64_t)0x7FFFFFFF - 2 * kPolRows)
    return fail(-1, who, "n " + to_string(n) + " is empty (<= 0) or above what 32 bits index");
  const int64_t nrb = (n + kPolRows - 1) / kPolRows;
  return kDiagLine * (nrb + (nrb > kDiagChunk ? (nrb + kDiagChunk - 1) / kDiagChunk : 0));
}
int64_t satrl_ppo_diagnostics_scratch(int64_t n) { return diag_scratch(__func__, n); }

int satrl_ppo_diagnostics(int H, int64_t n, const float* src, const int64_t* idx, const float* P, float epsilon,
                          float max_action, double* sums, double* scratch, int64_t scratch_len, float* rows_out,
                          void* stream) {
  if (int rc = refuse(__func__, H, kAnyH, n, "n", 0, SATRL_PTRS(src, P, sums, scratch))) return rc;
  const int64_t need = diag_scratch(__func__, n);
  if (need < 0) return -1;
  if (scratch_len < need)
    return fail(-1, __func__, "scratch holds " + to_string(scratch_len) + " f64, n " + to_string(n) + " needs " +
                             to_string(need));
  const int64_t nrb = (n + kPolRows - 1) / kPolRows;
  const char* who = __func__;
  if (int rc = with_width<kPolNW>(H, [&](auto w) {
        using W = decltype(w);
        return launch(who, diag_kernel<W::H, W::NW>, 2 * nrb, W::NW * 64, stream, (int)n, src, idx, P, epsilon,
                      max_action, scratch, rows_out);
      }))
    return rc;
  const double* lines = scratch;
  int64_t nl = nrb;
  if (nrb > kDiagChunk) {                                          // first level: a line per chunk of blocks
    double* l1 = scratch + nrb * kDiagLine;
    nl = (nrb + kDiagChunk - 1) / kDiagChunk;
    if (int rc = launch(who, diag_reduce_kernel, nl, 1024, stream, lines, nrb, kDiagChunk, l1, 0)) return rc;
    lines = l1;
  }
  return launch(who, diag_reduce_kernel, 1, 1024, stream, lines, nl, (int)nl, sums, 1);
}

int satrl_ppo_tanh(int64_t n, const float* x, float* y, void* stream) {
  if (n <= 0) return fail(-1, __func__, "n " + to_string(n) + " <= 0");
  if (int rc = null_arg(__func__, SATRL_PTRS(x, y))) return rc;
  return launch(__func__, tanh_kernel, (n + 255) / 256, 256, stream, n, x, y);
}

int satrl_tanh_forms(const float* x, float* y, int64_t n, int form, void* stream) {
  if (n <= 0 || n % 8 != 0) return fail(-1, __func__, "n " + to_string(n) + " is not a positive multiple of 8");
  if (int rc = null_arg(__func__, SATRL_PTRS(x, y))) return rc;
  if (int rc = outside(__func__, "form", form, 0, 1)) return rc;
  const int64_t n8 = n / 8;
  return launch(__func__, form == 0 ? tanh_forms_kernel<0> : tanh_forms_kernel<1>, (n8 + 255) / 256, 256, stream, n8, x,
                y);
}

// live launch spans (span_probe.h): the probe buffer, its bump pointer and
// the launch log, host state of the library (one probe per process)
int satrl_span_probe(void* buf, int64_t bytes, void* stream) {
  if ((buf == nullptr) != (bytes == 0) || bytes < 0)
    return fail(-1, __func__, "a buffer without bytes, bytes without a buffer, or bytes < 0");
  g_span.buf = static_cast<unsigned long long*>(buf);
  g_span.words = bytes / 8;
  if (!buf) return 0;                                              // stop: the log stays readable
  g_span.used = 0;
  g_span.log.clear();
  if (hipMemsetAsync(buf, 0, (size_t)bytes, (hipStream_t)stream) != hipSuccess) {
    g_span = SpanState{};
    return hip_failed(__func__, "hipMemsetAsync");
  }
  return 0;
}

int64_t satrl_span_probe_launches(void) { return (int64_t)g_span.log.size(); }

int satrl_span_probe_launch(int64_t i, int* kind, int64_t* word_offset, int64_t* waves) {
  if (i < 0 || i >= (int64_t)g_span.log.size())
    return fail(-1, __func__, "launch " + to_string(i) + " of " + to_string(g_span.log.size()) + " logged");
  if (int rc = null_arg(__func__, SATRL_PTRS(kind, word_offset, waves))) return rc;
  *kind = g_span.log[(size_t)i].kind;
  *word_offset = g_span.log[(size_t)i].off;
  *waves = g_span.log[(size_t)i].waves;
  return 0;
}

const char* satrl_ppo_last_error(void) { return satrl_err::slot.c_str(); }

}  // extern "C"


#ifdef SATRL_PHASE_PROBE
extern "C" int satrl_probe_read(unsigned long long* out) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_probe), sizeof(g_probe)) == hipSuccess ? 0 : -1;
}
#endif
