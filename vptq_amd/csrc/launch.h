// Host-side plumbing every launcher shares: the current device's slot and CU count, the > 64 KiB dynamic-LDS opt-in, and the
// writer of the *_instance texts.
#pragma once
#include <atomic>
#include <stdarg.h>
#include <stdio.h>
#include <hip/hip_runtime.h>

#include "../../include/vptq_hip.h"
#include "tune_env.h"

namespace vptq {

// Per-device state is kept in tables of kMaxDevices; the current device's index into them - 0 where there is no device
// (the host-only queries) or its ordinal is past the table
constexpr int kMaxDevices = 64;
inline int device_slot() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) dev = 0;
  return dev;
}

// CUs of the current device, looked up once per device; 256 (MI355X) where there is no device to ask - the host-only
// queries (kernel names, chain plans, instances) then answer for that
inline int device_cus() {
  static std::atomic<int> cus[kMaxDevices];
  const int dev = device_slot();
  if (!cus[dev]) {
    hipDeviceProp_t p;
    cus[dev] = hipGetDeviceProperties(&p, dev) == hipSuccess && p.multiProcessorCount > 0 ? p.multiProcessorCount : 256;
  }
  return cus[dev];
}

// More than 64 KiB of dynamic LDS must be allowed per kernel and device: the first launch of KERN on the current device sets the
// limit to `bytes` (benign race: idempotent).  A failure is returned and not remembered - the next call tries again.  The flags
// belong to the KERNEL (a template argument), not to its type: every instantiation of one kernel template has the same type.
template <auto KERN>
inline hipError_t allow_dynamic_lds(int bytes) {
  static std::atomic<bool> done[kMaxDevices];
  std::atomic<bool>& d = done[device_slot()];
  if (d) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute((const void*)KERN, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e == hipSuccess) d = true;
  return e;
}

inline const char* dt_text(bool f16) { return f16 ? "f16" : "bf16"; }

// The text of a *_instance query, appended piece by piece; text_done: 0, or -2 where the buffer was too small
struct Text {
  char* buf; size_t bytes, used; bool fits;
  void add(const char* fmt, ...) __attribute__((format(printf, 2, 3))) {
    if (!fits) return;
    va_list ap;
    va_start(ap, fmt);
    const int w = vsnprintf(buf + used, bytes - used, fmt, ap);
    va_end(ap);
    if (w < 0 || (size_t)w >= bytes - used) { fits = false; return; }
    used += (size_t)w;
  }
};
inline int text_done(const Text& t) { return t.fits ? 0 : -2; }

}  // namespace vptq
