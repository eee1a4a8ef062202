// The device primitives every stage stands on, handed the caller's arrays (diagnostics; tests/test_gpu_prims.py): the
// exclusive scan behind Engine::scan / scan2 in both of its forms and the small-batch path's single-block scan
// (kernels.hip), the 64-bit offsets of a list of lengths and the stable multi-key sort (device_prims.hpp).  An entry
// returns the device's raw answer; the comparison with a reference is the caller's.  (A .hip file: KeySort::run
// launches kernels.)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "device_prims.hpp"
#include "engine.hpp"

using namespace impg;

namespace {

// a stream of the entry's own: synchronised and destroyed on every path.  Declared after the buffers the stream's work
// uses, so that it is waited for before they are freed.
struct OwnStream {
  hipStream_t s = nullptr;
  OwnStream() { IMPG_HIP(hipStreamCreate(&s)); }
  ~OwnStream() {
    (void)hipStreamSynchronize(s);
    (void)hipStreamDestroy(s);
  }
  OwnStream(const OwnStream &) = delete;
  OwnStream &operator=(const OwnStream &) = delete;
};

constexpr uint32_t GUARD_WORDS = 64, GUARD = 0xA5A5A5A5u;

void check_guard(const std::vector<uint32_t> &h, size_t from, size_t to, const char *name) {
  for (size_t i = from; i < to; i++)
    if (h[i] != GUARD) throw Error{IMPG_E_INVALID, std::string("scan: the guard ") + name + " changed at word " + std::to_string(i - from)};
}

}  // namespace

extern "C" {

int impg_gpu_selftest_scan(int device, int which, const uint32_t *in, uint32_t n, uint32_t in_shift, uint32_t out_shift, uint32_t *out,
                           uint64_t *total, uint32_t *info) {
  IMPG_TRY
  if (which != 0 && which != 1) throw Error{IMPG_E_INVALID, "which is 0 (launch_exclusive_scan) or 1 (launch_small_scan)"};
  if (!in || !out || !total || !info || n == 0) throw Error{IMPG_E_INVALID, "scan: n > 0 items, and every array"};
  if (which == 1 && n > 1024) throw Error{IMPG_E_INVALID, "the small scan takes n <= 1024"};
  if (in_shift > 4 || out_shift > 4) throw Error{IMPG_E_INVALID, "a shift is 0 .. 4 words"};
  IMPG_HIP(hipSetDevice(device));
  // in: [in_shift words | n items];  out: [64 words | out_shift words | n items | 64 guard words] -- the 64 words in
  // front of the items are the front guard, and the items start out_shift words behind a 256-byte boundary;
  // scratch: [scan_scratch_bytes(n) | 64 guard words]
  const size_t out_front = GUARD_WORDS + out_shift, out_words = out_front + n + GUARD_WORDS;
  const size_t scratch_words = (scan_scratch_bytes(n) + 3) / 4, scratch_all = scratch_words + GUARD_WORDS;
  DevBuf d_in, d_out, d_scratch, d_total;
  d_in.reserve(((size_t)in_shift + n) * 4); d_out.reserve(out_words * 4); d_scratch.reserve(scratch_all * 4); d_total.reserve(8);
  for (const DevBuf *b : {&d_in, &d_out, &d_scratch, &d_total})
    if (reinterpret_cast<uintptr_t>(b->p) & 255u) throw Error{IMPG_E_INVALID, "scan: an allocation is not 256-byte aligned"};
  const uint32_t *p_in = d_in.as<uint32_t>() + in_shift;
  uint32_t *p_out = d_out.as<uint32_t>() + out_front;
  OwnStream st;
  hipStream_t s = st.s;
  IMPG_HIP(hipMemsetAsync(d_in.p, 0xA5, d_in.cap, s));
  IMPG_HIP(hipMemsetAsync(d_out.p, 0xA5, out_words * 4, s));
  IMPG_HIP(hipMemsetAsync(d_scratch.p, 0xA5, scratch_all * 4, s));  // (the engine's scratch is not cleared between scans either)
  IMPG_HIP(hipMemsetAsync(d_total.p, 0xA5, 8, s));
  IMPG_HIP(hipMemcpyAsync(d_in.as<uint32_t>() + in_shift, in, (size_t)n * 4, hipMemcpyHostToDevice, s));
  int form = 2;  // (the small scan)
  if (which == 0) form = launch_exclusive_scan(p_in, p_out, n, d_scratch.as<unsigned long long>(), d_total.as<unsigned long long>(), s);
  else launch_small_scan(p_in, n, p_out, d_total.as<uint32_t>(), s);
  IMPG_HIP(hipGetLastError());
  std::vector<uint32_t> h_out(out_words), h_scratch(scratch_all);
  unsigned long long h_total = 0;
  IMPG_HIP(hipMemcpyAsync(h_out.data(), d_out.p, out_words * 4, hipMemcpyDeviceToHost, s));
  IMPG_HIP(hipMemcpyAsync(h_scratch.data(), d_scratch.p, scratch_all * 4, hipMemcpyDeviceToHost, s));
  IMPG_HIP(hipMemcpyAsync(&h_total, d_total.p, which == 0 ? 8 : 4, hipMemcpyDeviceToHost, s));
  IMPG_HIP(hipStreamSynchronize(s));
  std::copy(h_out.begin() + out_front, h_out.begin() + out_front + n, out);
  *total = h_total;
  info[0] = (uint32_t)form;
  info[1] = (uint32_t)(reinterpret_cast<uintptr_t>(p_in) & 15u);
  info[2] = (uint32_t)(reinterpret_cast<uintptr_t>(p_out) & 15u);
  scan_tile_sizes(&info[3], &info[4]);
  check_guard(h_out, 0, out_front, "in front of out");
  check_guard(h_out, out_front + n, out_words, "behind out");
  check_guard(h_scratch, scratch_words, scratch_all, "behind the scratch");
  return IMPG_OK;
  IMPG_CATCH
}

int impg_gpu_selftest_offsets(int device, const uint32_t *len, uint32_t n, int with_host_copy, uint64_t *off, uint64_t *total) {
  IMPG_TRY
  if (!len || !off || !total || n == 0) throw Error{IMPG_E_INVALID, "offsets: n > 0 lengths, and every array"};
  IMPG_HIP(hipSetDevice(device));
  DevBuf d_len, d_off, tmp;
  d_len.reserve((size_t)n * 4); d_off.reserve((size_t)n * 8);
  OwnStream st;
  hipStream_t s = st.s;
  IMPG_HIP(hipMemcpyAsync(d_len.p, len, (size_t)n * 4, hipMemcpyHostToDevice, s));
  IMPG_HIP(hipMemsetAsync(d_off.p, 0xA5, (size_t)n * 8, s));
  if (with_host_copy) {  // (the text stages' form: the offsets come home with the total's wait)
    std::vector<unsigned long long> h_off(n, ~0ull);
    *total = prims::offsets_and_total(tmp, (const uint32_t *)d_len.as<uint32_t>(), d_off.as<unsigned long long>(), n, s, h_off.data());
    std::copy(h_off.begin(), h_off.end(), off);
  } else {
    *total = prims::offsets_and_total(tmp, d_len.as<uint32_t>(), d_off.as<unsigned long long>(), n, s);
    IMPG_HIP(hipMemcpyAsync(off, d_off.p, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    IMPG_HIP(hipStreamSynchronize(s));
  }
  return IMPG_OK;
  IMPG_CATCH
}

int impg_gpu_selftest_key_sort(int device, uint32_t n_keys, const uint32_t *perm, uint32_t m, int first_in_order,
                               const impg_gpu_sort_pass_t *passes, uint32_t n_passes, uint32_t *order, void *sorted_keys) {
  IMPG_TRY
  if (!perm || !passes || !order || !sorted_keys) throw Error{IMPG_E_INVALID, "key sort: every array"};
  if (n_passes < 1 || n_passes > 3) throw Error{IMPG_E_INVALID, "key sort: 1 .. 3 passes"};
  if (m == 0 || m > n_keys) throw Error{IMPG_E_INVALID, "key sort: 0 < m <= n_keys"};
  for (uint32_t k = 0; k < n_passes; k++)
    if (!passes[k].keys || passes[k].bits < 1 || passes[k].bits > (passes[k].wide ? 64u : 32u))
      throw Error{IMPG_E_INVALID, "key sort: a pass has keys and 1 .. 32 (wide: 64) bits"};
  for (uint32_t i = 0; i < m; i++) {  // (the gathers read keys[perm[i]])
    if (perm[i] >= n_keys) throw Error{IMPG_E_INVALID, "key sort: perm names a row >= n_keys"};
    if (first_in_order && perm[i] != i) throw Error{IMPG_E_INVALID, "key sort: first_in_order takes the identity"};
  }
  if (first_in_order && m != n_keys) throw Error{IMPG_E_INVALID, "key sort: first_in_order takes m = n_keys"};
  IMPG_HIP(hipSetDevice(device));
  // the passes' keys are copied: a gathering pass sorts back into the pass's own array
  DevBuf d_keys[3];
  prims::KeySort ks;
  OwnStream st;
  hipStream_t s = st.s;
  prims::SortPass sp[3];
  for (uint32_t k = 0; k < n_passes; k++) {
    const size_t bytes = (size_t)n_keys * (passes[k].wide ? 8 : 4);
    d_keys[k].reserve(bytes);
    IMPG_HIP(hipMemcpyAsync(d_keys[k].p, passes[k].keys, bytes, hipMemcpyHostToDevice, s));
    sp[k] = prims::SortPass{d_keys[k].p, passes[k].wide != 0, passes[k].bits};
  }
  ks.perm.reserve((size_t)m * 4);
  IMPG_HIP(hipMemcpyAsync(ks.perm.p, perm, (size_t)m * 4, hipMemcpyHostToDevice, s));
  switch (n_passes) {
    case 1: ks.run({sp[0]}, first_in_order != 0, m, s); break;
    case 2: ks.run({sp[0], sp[1]}, first_in_order != 0, m, s); break;
    default: ks.run({sp[0], sp[1], sp[2]}, first_in_order != 0, m, s); break;
  }
  IMPG_HIP(hipGetLastError());
  IMPG_HIP(hipMemcpyAsync(order, ks.order, (size_t)m * 4, hipMemcpyDeviceToHost, s));
  IMPG_HIP(hipMemcpyAsync(sorted_keys, ks.sorted_keys, (size_t)m * (passes[n_passes - 1].wide ? 8 : 4), hipMemcpyDeviceToHost, s));
  IMPG_HIP(hipStreamSynchronize(s));
  return IMPG_OK;
  IMPG_CATCH
}

}  // extern "C"
