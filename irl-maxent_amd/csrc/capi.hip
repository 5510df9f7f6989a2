// Error reporting and version of the irlmx C ABI, and the host utilities the
// launch paths share.  No C++ exception crosses the ABI: failures return a
// negative code and leave a thread-local message.

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "cluster.h"
#include "common.h"

namespace irlmx {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int hip_fail(hipError_t e, const char* what) {
  set_error("%s: %s (%d)", what, hipGetErrorString(e), (int)e);
  return IRLMX_EHIP;
}

int env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return (e && *e) ? atoi(e) : dflt;
}

int device_cus() {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
  return cus;
}

int launch_capacity(const void* fn, int threads) {
  const int f_cus = env_int("IRLMX_PLAN_CUS", 0), f_per = env_int("IRLMX_PLAN_GRID_PER_CU", 0);
  if (f_cus > 0 && f_per > 0) return f_cus * f_per;
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, threads, 0) != hipSuccess) return 0;
  return device_cus() * per_cu;
}

LaunchTestKnobs launch_test_knobs() {
  const int tmo_ms = env_int("IRLMX_TEST_EXCHANGE_TIMEOUT_MS", 0);
  return LaunchTestKnobs{env_int("IRLMX_TEST_NOT_RESIDENT", 0) ? 1 : 0, env_int("IRLMX_TEST_DROP_TILE", -1),
                         tmo_ms > 0 ? (unsigned long long)tmo_ms * 100000ull : kGatherTicks};
}

static std::atomic<long long> g_counters[IRLMX_COUNTERS_LEN];

void count_event(int which) {
  if (which >= 0 && which < IRLMX_COUNTERS_LEN) g_counters[which].fetch_add(1, std::memory_order_relaxed);
}

void note_exchange_timeout(const char* shape) {
  static std::atomic<bool> told{false};
  if (!told.exchange(true))
    fprintf(stderr,
            "irlmx: %s shape: an exchange timed out (a workgroup descheduled or a lost granule); the call was rerun "
            "on the per-sweep shape (counter rerun_timeout; IRLMX_STRICT_EXCHANGE=1 makes it an error)\n", shape);
}

int grid_launch_outcome(int* err_words, const char* label, hipStream_t st) {
  char what[64];
  int err = 0;
  hipError_t e = hipMemcpyAsync(&err, err_words, sizeof(int), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) {
    snprintf(what, sizeof(what), "%s sync", label);
    return hip_fail(e, what);
  }
  if (!err) return 0;
  const bool timeout = !(err & kErrNotResident);
  if (timeout && env_int("IRLMX_STRICT_EXCHANGE", 0)) {
    set_error("%s shape: exchange timed out (workgroups not co-resident?)", label);
    return IRLMX_EHIP;
  }
  if (timeout) note_exchange_timeout(label);
  count_event(timeout ? IRLMX_CTR_RERUN_TIMEOUT : IRLMX_CTR_RERUN_NOT_RESIDENT);
  e = hipMemsetAsync(err_words, 0, 4 * sizeof(int), st);
  if (e == hipSuccess) return kClusterNotResident;
  snprintf(what, sizeof(what), "%s err reset", label);
  return hip_fail(e, what);
}

__global__ void numpy_math_kernel(int op, const double* __restrict__ x, double* __restrict__ y, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    y[i] = op == IRLMX_NPMATH_EXP ? np_exp(x[i]) : np_log(x[i]);
}

static std::vector<DcheckTake>& dcheck_registry() {
  static std::vector<DcheckTake> r;
  return r;
}

bool register_dcheck(DcheckTake take) {
  dcheck_registry().push_back(take);
  return true;
}

}  // namespace irlmx

extern "C" int irlmx_device_checks_enabled(void) { return IRLMX_DEVICE_CHECKS; }

extern "C" int64_t irlmx_device_check_failures(void) {
  if (!IRLMX_DEVICE_CHECKS) return 0;
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  unsigned v = 0;
  for (auto take : irlmx::dcheck_registry()) v |= take();
  return (int64_t)v;
}

extern "C" int irlmx_abi_version(void) { return IRLMX_ABI_VERSION; }

extern "C" int irlmx_numpy_math(int32_t op, const double* x, double* y, int64_t n, void* stream) {
  if (op != IRLMX_NPMATH_EXP && op != IRLMX_NPMATH_LOG) {
    irlmx::set_error("unknown op %d", op);
    return IRLMX_EINVAL;
  }
  if (n < 0) {
    irlmx::set_error("n = %lld < 0", (long long)n);
    return IRLMX_EINVAL;
  }
  if (n == 0) return IRLMX_OK;
  if (!x || !y) {
    irlmx::set_error("x or y is NULL");
    return IRLMX_EINVAL;
  }
  const int64_t blocks = (n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096;
  hipLaunchKernelGGL(irlmx::numpy_math_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, op, x, y, n);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return irlmx::hip_fail(e, "numpy_math_kernel");
  return IRLMX_OK;
}

extern "C" const char* irlmx_last_error(void) { return irlmx::g_err; }

extern "C" int irlmx_counters(int64_t* out, int32_t n) {
  if (out)
    for (int i = 0; i < n && i < IRLMX_COUNTERS_LEN; ++i)
      out[i] = irlmx::g_counters[i].load(std::memory_order_relaxed);
  return IRLMX_COUNTERS_LEN;
}
