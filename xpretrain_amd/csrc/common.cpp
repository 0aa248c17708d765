// Host-side helpers shared by every translation unit of libxpretrain_hip.so.
#include "common.h"
#include <string.h>
#include <map>
#include <mutex>

static thread_local char g_err[512] = "";

void xp_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

extern "C" const char* xp_last_error(void) { return g_err; }

// XPRETRAIN_DEBUG=flag[,flag...]: the one environment variable of the debug / test facilities (read at every query, so a tool can
// flip a flag between two calls).  C side: gemm_no_glds, gemm_slow_epi (128x128 family: register-staged loader / generic epilogue --
// tools/race_repro.py), dw_tile_major (split-K launches on the (tile, z) grid instead of the chunk-major 1-D grid: the bit-identity
// test), attn_bwd_split (the dQ / dK-dV kernel pair instead of the fused attention backward: A/B and the cross-check test).
// Python side (xpretrain_amd/_lib.py): sync, op_by_op, no_comm.
bool xp_debug_flag(const char* name) {
  const char* env = getenv("XPRETRAIN_DEBUG");
  if (!env || !*env) return false;
  const size_t n = strlen(name);
  for (const char* p = env; (p = strstr(p, name)) != nullptr; p += n) {
    const bool left = p == env || p[-1] == ',', right = p[n] == '\0' || p[n] == ',';
    if (left && right) return true;
  }
  return false;
}
extern "C" int xp_abi_version(void) { return XP_ABI_VERSION; }

// CUs of the current device; with a kernel, after granting it `lds_bytes` of dynamic LDS there -- once per (kernel, device), under one
// lock (the forward and the autograd thread may both arrive first).  0 (message set): no current device, or the opt-in was refused.
int xp_device_cus(const void* kernel, int lds_bytes) {
  static std::mutex mu;
  static std::map<std::pair<const void*, int>, int> known;      // (kernel or NULL, device) -> CU count, -1: opt-in refused
  int dev = -1, n = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0) { xp_set_error("no current HIP device"); return 0; }
  std::lock_guard<std::mutex> lock(mu);
  int& cus = known[{kernel, dev}];
  if (!cus && kernel && hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes) != hipSuccess) cus = -1;
  if (!cus) cus = hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0 ? n : 256;
  if (cus < 0) xp_set_error("device %d refused a kernel's dynamic-LDS opt-in of %d bytes", dev, lds_bytes);
  return cus > 0 ? cus : 0;
}
