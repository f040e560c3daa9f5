// debug_tap.h — what the unit-test taps share (gemm_debug.hip, ws_debug.hip, small_debug.hip): the holder of a tap's device copies, the
// bound check of one host array, and the copies to the device and back.  Host code only.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/orl_engine.h"

namespace orl {

int fail(const std::string& msg);      // engine.hip: sets orl_last_error(), returns -1

// device arrays of one tap call: freed on every return path.  `who` names the entry point in the error text.
struct TapDev {
  std::vector<void*> ptrs;
  ~TapDev() { for (void* q : ptrs) hipFree(q); }
  template <class T>
  int alloc(T** p, size_t count, const char* who) {
    if (hipMalloc((void**)p, sizeof(T) * count) != hipSuccess) return fail(std::string(who) + " device: hipMalloc failed");
    ptrs.push_back(*p);
    return 0;
  }
};

// One array of a tap: `ext` elements per (problem, slab) starting at off + z0 s0 + z1 s1 + ks ks must lie inside [0, n), and the
// problems / slabs of a result must not overlap.  nslab 0: a tap without slabs (it says so in the overlap text).
static inline bool tap_fits(const orl_gemm_buf& b, const std::string& name, long ext, int nz0, int nz1, int nslab, bool result, std::string& why) {
  if (!b.host) { why = name + " is required"; return false; }
  if (b.n <= 0 || b.n > (1L << 28)) { why = name + ": bad element count"; return false; }
  if (b.off < 0 || b.s0 < 0 || b.s1 < 0 || b.ks < 0 || b.pitch < 0) { why = name + ": negative offset, pitch or stride"; return false; }
  if (ext < 1) { why = name + ": empty extent"; return false; }
  if (result && ((nz0 > 1 && b.s0 < ext) || (nz1 > 1 && b.s1 < ext) || (nslab > 1 && b.ks < ext))) {
    why = name + (nslab ? ": problems or slabs of a result overlap" : ": problems of a result overlap");
    return false;
  }
  const long last = b.off + (long)(nz0 - 1) * b.s0 + (long)(nz1 - 1) * b.s1 + (nslab > 1 ? (long)(nslab - 1) * b.ks : 0) + ext;
  if (last > b.n) { why = name + ": the array is shorter than its offset, strides and pitch need"; return false; }
  return true;
}

// The arrays of a call as the copies walk them: n 4-byte elements from `src` to a device copy (src null: none), and the copy back to
// `back` after the launch (null: not read back).
struct TapArray { const void* src; void* back; long n; };

// base[i] = the device copy of arrays[i], or null
static inline int tap_upload(TapDev& dev, const std::vector<TapArray>& arrays, char** base, const char* who) {
  for (size_t i = 0; i < arrays.size(); ++i) {
    base[i] = nullptr;
    const TapArray& t = arrays[i];
    if (!t.src) continue;
    float* d = nullptr;
    if (dev.alloc(&d, (size_t)t.n, who)) return -1;
    base[i] = (char*)d;
    if (hipMemcpy(d, t.src, sizeof(float) * t.n, hipMemcpyHostToDevice) != hipSuccess) return fail(std::string(who) + " device: copy to the device failed");
  }
  return 0;
}
static inline int tap_download(const std::vector<TapArray>& arrays, char* const* base, const char* who) {
  for (size_t i = 0; i < arrays.size(); ++i)
    if (base[i] && arrays[i].back && hipMemcpy(arrays[i].back, base[i], sizeof(float) * arrays[i].n, hipMemcpyDeviceToHost) != hipSuccess)
      return fail(std::string(who) + " device: copy from the device failed");
  return 0;
}

}  // namespace orl
