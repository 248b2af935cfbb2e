// Host-side runtime glue of liboct_hip.so: error reporting, version, device probing.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <mutex>
#include <set>
#include <utility>
#include "../../include/oct_hip.h"

static thread_local char g_err[512] = "";

void oct_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int oct_check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    oct_set_error("%s: launch failed: %s", what, hipGetErrorString(e));
    return OCT_E_LAUNCH;
  }
  return OCT_OK;
}

// hipFuncAttributeMaxDynamicSharedMemorySize is a per-device setting: remembered per (device, kernel), set under a lock
int oct_lds_optin(const void* kernel, int bytes) {
  static std::mutex mu;
  static std::set<std::pair<int, const void*>> done;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e == hipSuccess) {
    std::lock_guard<std::mutex> lock(mu);
    if (done.count({dev, kernel})) return OCT_OK;
    e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess) {
      done.insert({dev, kernel});
      return OCT_OK;
    }
  }
  (void)hipGetLastError();
  oct_set_error("opting a kernel in to %d bytes of LDS failed: %s", bytes, hipGetErrorString(e));
  return OCT_E_LAUNCH;
}

extern "C" {
const char* oct_version_string(void) { return "oct_hip 0.2.2 (gfx950)"; }
int oct_version(void) { return OCT_VERSION; }
int oct_get_last_error(char* buf, size_t len) {
  if (!buf || len == 0) return OCT_E_INVALID;
  strncpy(buf, g_err, len - 1);
  buf[len - 1] = 0;
  return OCT_OK;
}
int oct_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return n;
}
}
