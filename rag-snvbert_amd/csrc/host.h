// The host layer of libsnvrag's C entry points: argument checks, dispatch on the model width and
// the dynamic-LDS launch.  Host code only.  An entry point validates with the checks below and
// launches through SNV_LAUNCH_LDS; every failure goes through fail(), which records the text
// snvrag_last_error() returns.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <string>
#include <type_traits>
#include <utility>

namespace snvrag {

int fail(const char* where, const std::string& msg);

static inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }
static inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// every pointer is a multiple of n bytes (a null pointer is: whether it may be null is the
// business of SNV_CHECK_PTRS)
template <typename... P>
inline bool aligned(size_t n, const P*... p) { return (((uintptr_t)p % n == 0) && ...); }
template <typename... P>
inline bool non_null(const P*... p) { return ((p != nullptr) && ...); }

// f(std::integral_constant<int, D>{}) for the model widths D in {128, 256, 384}.  The caller
// refuses every other D first (tail.hip: tail_d_ok); a D that slipped through would run the 384
// instantiation
template <typename F>
inline auto dispatch_d(int D, F&& f) {
  switch (D) {
    case 128: return f(std::integral_constant<int, 128>{});
    case 256: return f(std::integral_constant<int, 256>{});
    default: return f(std::integral_constant<int, 384>{});
  }
}

// compute units of the current device (256 when the runtime cannot tell), cached per device
inline int cu_count() {
  static int n[16] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) dev = 0;
  if (n[dev] <= 0) {
    int v = 0;
    n[dev] = hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0 ? v : 256;
  }
  return n[dev];
}

// Raises the kernel's dynamic-LDS limit to lds_bytes (on every launch), launches and checks;
// returns 0, or fail(where, ...) with the runtime's text for a refused attribute or launch.
template <typename... KA, typename... A>
inline int launch_lds(const char* where, void (*kern)(KA...), dim3 grid, dim3 block, size_t lds_bytes, hipStream_t s,
                      A&&... args) {
  hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(kern, grid, block, lds_bytes, s, std::forward<A>(args)...);
    e = hipGetLastError();
  }
  return e == hipSuccess ? 0 : fail(where, hipGetErrorString(e));
}

}  // namespace snvrag

// ---- argument checks ----
// refuse the call unless cond holds: the text goes to snvrag_last_error() under the function's
// name (SNV_CHECK_AS: under the name given, for a helper that checks on an entry point's behalf)
#define SNV_CHECK_AS(where, cond, msg)                               \
  do {                                                               \
    if (!(cond)) return ::snvrag::fail((where), (msg));              \
  } while (0)
#define SNV_CHECK_ARG(cond, msg) SNV_CHECK_AS(__func__, cond, msg)
#define SNV_CHECK_PTRS(...) SNV_CHECK_ARG(::snvrag::non_null(__VA_ARGS__), "null pointer")
#define SNV_CHECK_ALIGN(n, msg, ...) SNV_CHECK_ARG(::snvrag::aligned((n), __VA_ARGS__), (msg))
// a row count the kernels carry as int
#define SNV_CHECK_M(M) SNV_CHECK_ARG((M) >= 0 && (M) < (1L << 31), "bad M")

// ---- runtime calls and launches ----
#define SNV_HIP(expr)                                                \
  do {                                                               \
    hipError_t e_ = (expr);                                          \
    if (e_ != hipSuccess)                                            \
      return ::snvrag::fail(__func__, hipGetErrorString(e_));        \
  } while (0)

// launch + error check (kernel launch errors surface via hipGetLastError)
#define SNV_LAUNCH_CHECK()                                           \
  do {                                                               \
    hipError_t e_ = hipGetLastError();                               \
    if (e_ != hipSuccess)                                            \
      return ::snvrag::fail(__func__, hipGetErrorString(e_));        \
  } while (0)

// launch_lds under the calling function's name, as SNV_HIP / SNV_LAUNCH_CHECK report
#define SNV_LAUNCH_LDS(kern, grid, block, lds_bytes, s, ...) \
  ::snvrag::launch_lds(__func__, (kern), (grid), (block), (lds_bytes), (s), __VA_ARGS__)
