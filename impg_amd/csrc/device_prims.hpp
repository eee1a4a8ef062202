// The rocPRIM scans and sorts of the device files, over a temp buffer the caller owns: a call asks the library how much temp
// storage it wants, grows the buffer only when that is more than it holds (never below 256 bytes) and runs on the caller's
// stream.  The iterator and count types are the caller's own, so a call instantiates the library kernels the spelled-out form did.
// Also what more than one device file wants besides: the grid and key-width arithmetic, the two helper kernels (internal
// linkage: every translation unit has its own copy), the stable multi-key sort over them and the offsets of a list of lengths.
#pragma once
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <iterator>

#include "impg_internal.hpp"
#include "kernels.hpp"

namespace impg {
namespace prims {

// ---- arithmetic: one meaning per name in every device file (each says `using prims::cdiv;` for what it calls) ----------
inline uint32_t cdiv(uint64_t a, uint32_t b) { return (uint32_t)((a + b - 1) / b); }  // blocks of b that cover a items: 0 for none
inline uint32_t cdiv1(size_t a, uint32_t b) { return (uint32_t)std::max<size_t>((a + b - 1) / b, 1); }  // ... and never 0: a grid that always launches
inline unsigned bits_for(uint64_t n) {  // key bits that index n values (0 .. n - 1), at least 1
  unsigned b = 0;
  while ((1ull << b) < n) b++;
  return std::max(1u, b);
}
inline unsigned bits_upto(uint32_t v) {  // key bits that hold 0 .. v
  unsigned b = 1;
  while (b < 32 && (v >> b)) b++;
  return b;
}
__device__ __forceinline__ uint32_t ord_u32(int32_t v) { return (uint32_t)v ^ 0x80000000u; }  // order-preserving

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
// out[i] = in[0] (op) .. (op) in[i], op associative (it need not commute: the operands keep their order)
template <class In, class Out, class Op> inline void inclusive_scan(DevBuf &tmp, In in, Out out, size_t n, Op op, hipStream_t s) {
  size_t sb = 0;
  IMPG_HIP(rocprim::inclusive_scan(nullptr, sb, in, out, n, op, s));
  grow(tmp, sb);
  IMPG_HIP(rocprim::inclusive_scan(tmp.p, sb, in, out, n, op, s));
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

// off[i] = len[0] + .. + len[i - 1] in 64 bits, and their total (= off[n - 1] + len[n - 1], read back: the stream is
// synchronised before this returns).  n > 0.  h_off (optional): the n offsets for the host, home with the same wait.
// In: the caller's own pointer type (uint32_t *, const uint32_t *), so that the scan it instantiates is the one it had.
template <class In> inline unsigned long long offsets_and_total(DevBuf &tmp, In len, unsigned long long *off, uint32_t n, hipStream_t s,
                                                               unsigned long long *h_off = nullptr) {
  exclusive_sum(tmp, len, off, n, s);
  unsigned long long last_off = 0;
  uint32_t last_len = 0;
  if (h_off) IMPG_HIP(hipMemcpyAsync(h_off, off, (size_t)n * 8, hipMemcpyDeviceToHost, s));
  else IMPG_HIP(hipMemcpyAsync(&last_off, off + (n - 1), 8, hipMemcpyDeviceToHost, s));
  IMPG_HIP(hipMemcpyAsync(&last_len, len + (n - 1), 4, hipMemcpyDeviceToHost, s));
  IMPG_HIP(hipStreamSynchronize(s));
  return (h_off ? h_off[n - 1] : last_off) + last_len;
}

// ---- stable sort by several keys, least significant first ----------------------------------------------------------------
// A pass gathers its key through the current permutation into `stage` and radix-sorts (key, permutation) by the key's low
// `bits` bits (launch_sort_u32 / launch_sort_pairs, kernels.hip) back into the pass's own array, which the gather has read.
// first_in_order: perm is the identity, so the first pass sorts its keys where they stand, into `stage`.  The caller fills
// perm; after run(), order = the sorted permutation and sorted_keys = the last pass's keys in that order.  (run is a
// template so that the gather kernels exist only in the translation units that sort.)
struct SortPass { void *keys; bool wide; unsigned bits; };  // keys: at every element's own index, 32 or (wide) 64 bits each
struct KeySort {
  DevBuf perm, spare, stage, tmp;
  uint32_t *order = nullptr;
  const void *sorted_keys = nullptr;
  explicit KeySort(BufPool *pool = nullptr) { for (DevBuf *b : {&perm, &spare, &stage, &tmp}) b->pool = pool; }
  template <size_t N> void run(const SortPass (&passes)[N], bool first_in_order, uint32_t n, hipStream_t s) {
    typedef unsigned long long u64;
    spare.reserve((size_t)n * 4); stage.reserve((size_t)n * 8);
    tmp.reserve(std::max(sort_u32_scratch_bytes(n), sort_pairs_scratch_bytes(n)));
    uint32_t *in = perm.as<uint32_t>(), *out = spare.as<uint32_t>();
    for (const SortPass &p : passes) {
      const bool gather = !(first_in_order && &p == passes);
      void *src = gather ? stage.p : p.keys, *dst = gather ? p.keys : stage.p;
      if (gather && p.wide) gather_kernel<<<cdiv(n, 256), 256, 0, s>>>((const u64 *)p.keys, in, n, (u64 *)src);
      else if (gather) gather_kernel<<<cdiv(n, 256), 256, 0, s>>>((const uint32_t *)p.keys, in, n, (uint32_t *)src);
      if (p.wide) launch_sort_pairs(tmp.p, tmp.cap, (const u64 *)src, (u64 *)dst, in, out, n, p.bits, s);
      else launch_sort_u32(tmp.p, tmp.cap, (const uint32_t *)src, (uint32_t *)dst, in, out, n, s, 0, p.bits);
      sorted_keys = dst;
      std::swap(in, out);
    }
    order = in;
  }
};

}  // namespace prims
}  // namespace impg
