// satrl_error.h -- the error slot of the satrl_* C ABI (include/satrl_ppo.h,
// satrl_peer.h, satrl_rollout.h), the refusal that fills it, and the checked
// launch of the two hipcc translation units.  The slot is a C++17 inline
// variable: ppo_kernels.hip, rollout_kernels.hip and satenv_cpu.cpp share one
// instance per thread inside libsatrl.so, and both satrl_last_error and
// satrl_ppo_last_error return it.  The satenv_* and satenv_cpu_* ABIs keep
// their own slots.  An extern "C" entry point passes __func__ as its name.
#pragma once
#include <cstdint>
#include <initializer_list>
#include <string>

namespace satrl_err {

inline thread_local std::string slot;

// A refusal of entry point `who`: "<who>: <why>" in the slot, `code` returned.
// Only a failing call gets here, so a successful one forms no string.
inline int fail(int code, const char* who, const std::string& why) {
  slot.assign(who).append(": ").append(why);
  return code;
}

// The pointers an entry point requires with their parameter names, "a, b, c":
// SATRL_PTRS(src, P, W2X).  null_arg refuses the first NULL one by its name
// and returns 0 when none is.
struct Ptrs {
  const char* names;
  std::initializer_list<const void*> ptrs;
};
#define SATRL_PTRS(...) satrl_err::Ptrs{#__VA_ARGS__, {__VA_ARGS__}}
inline int null_arg(const char* who, const Ptrs& need) {
  const char* name = need.names;
  for (const void* p : need.ptrs) {
    const char* end = name;
    while (*end && *end != ',') ++end;
    if (!p) return fail(-1, who, std::string(name, end) + " is NULL");
    for (name = end; *name == ',' || *name == ' ';) ++name;
  }
  return 0;
}

#ifdef __HIPCC__
// after `who`'s launch: 0, or -2 with HIP's text
inline int launched(const char* who) {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail(-2, who, hipGetErrorString(e));
}
// a block count as a grid: refused when it does not fit a grid dimension
inline int grid_of(const char* who, int64_t blocks, dim3* g) {
  if (blocks > 0x7FFFFFFF) return fail(-1, who, std::to_string(blocks) + " blocks are too large for one grid");
  *g = dim3((unsigned)blocks);
  return 0;
}
// one launch of kernel k on `blocks` workgroups of `threads` threads: the grid checked, then the launch
template <class... KA, class... A>
int launch(const char* who, void (*k)(KA...), int64_t blocks, int threads, void* stream, A... args) {
  dim3 g;
  if (int rc = grid_of(who, blocks, &g)) return rc;
  hipLaunchKernelGGL(k, g, dim3(threads), 0, (hipStream_t)stream, args...);
  return launched(who);
}
#endif

}  // namespace satrl_err
