// The rocPRIM scans and sorts of the device files, over a temp buffer the caller owns: a call asks the library how much temp
// storage it wants, grows the buffer only when that is more than it holds (never below 256 bytes) and runs on the caller's
// stream.  The iterator and count types are the caller's own, so a call instantiates the library kernels the spelled-out form did.
// Also the two helper kernels more than one device file wants (internal linkage: every translation unit has its own copy).
#pragma once
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <iterator>

#include "impg_internal.hpp"

namespace impg {
namespace prims {

template <class It> using value_of = typename std::iterator_traits<It>::value_type;
inline void grow(DevBuf &tmp, size_t bytes) { tmp.reserve(std::max<size_t>(bytes, 256)); }

// out[i] = in[0] + .. + in[i - 1], summed in out's type (uint32 -> uint32, uint32 -> uint64)
template <class In, class Out> inline void exclusive_sum(DevBuf &tmp, In in, Out out, size_t n, hipStream_t s) {
  typedef value_of<Out> T;
  size_t sb = 0;
  IMPG_HIP(rocprim::exclusive_scan(nullptr, sb, in, out, T(0), n, rocprim::plus<T>(), s));
  grow(tmp, sb);
  IMPG_HIP(rocprim::exclusive_scan(tmp.p, sb, in, out, T(0), n, rocprim::plus<T>(), s));
}
// out[i] = max(in[0 .. i])
template <class In, class Out> inline void inclusive_max(DevBuf &tmp, In in, Out out, size_t n, hipStream_t s) {
  size_t sb = 0;
  IMPG_HIP(rocprim::inclusive_scan(nullptr, sb, in, out, n, rocprim::maximum<value_of<Out>>(), s));
  grow(tmp, sb);
  IMPG_HIP(rocprim::inclusive_scan(tmp.p, sb, in, out, n, rocprim::maximum<value_of<Out>>(), s));
}
// Stable sort of (key, value) pairs by the keys' bits [begin_bit, end_bit); query and sort also apart: the engine sizes its scratch up front.
template <class KI, class KO, class VI, class VO, class Size> inline size_t radix_sort_pairs_bytes(Size n, unsigned begin_bit, unsigned end_bit) {
  size_t sb = 0;
  IMPG_HIP(rocprim::radix_sort_pairs(nullptr, sb, KI(), KO(), VI(), VO(), n, begin_bit, end_bit, (hipStream_t)0));  // (null pointers of the sort's types)
  return sb;
}
template <class KI, class KO, class VI, class VO, class Size>
inline void radix_sort_pairs(void *tmp, size_t tmp_bytes, KI kin, KO kout, VI vin, VO vout, Size n, unsigned begin_bit, unsigned end_bit, hipStream_t s) {
  IMPG_HIP(rocprim::radix_sort_pairs(tmp, tmp_bytes, kin, kout, vin, vout, n, begin_bit, end_bit, s));
}
template <class KI, class KO, class VI, class VO, class Size>
inline void radix_sort_pairs(DevBuf &tmp, KI kin, KO kout, VI vin, VO vout, Size n, unsigned begin_bit, unsigned end_bit, hipStream_t s) {
  const size_t sb = radix_sort_pairs_bytes<KI, KO, VI, VO>(n, begin_bit, end_bit);
  grow(tmp, sb);
  radix_sort_pairs(tmp.p, sb, kin, kout, vin, vout, n, begin_bit, end_bit, s);
}

namespace {
template <class T> __global__ __launch_bounds__(256) void iota_kernel(T *v, uint32_t n) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < n) v[i] = i;
}
template <class T>
__global__ __launch_bounds__(256) void gather_kernel(const T *__restrict__ src, const uint32_t *__restrict__ idx, uint32_t n, T *__restrict__ dst) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < n) dst[i] = src[idx[i]];
}
}  // namespace

}  // namespace prims
}  // namespace impg
