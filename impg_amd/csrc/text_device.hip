// The host side of the device text writers (text_device.hpp): the upload of a chunk's name / shift / range-name tables and
// the piece loop that streams finished text through two pinned buffers.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "text_device.hpp"

namespace impg {

// The name / shift / range-name tables of a chunk (text_device.hpp)
TextTableBufs::TextTableBufs(Engine &E, const impg_gpu_index &ix, uint32_t n_ranges, const std::vector<std::string> &rnames, bool original_coords,
                             bool with_lengths) {
  hipStream_t s = E.stream;
  noff.assign(1, 0);
  for (const std::string &nm : ix.seq.names) {
    nshift.push_back(put_original_name(nb, nm, original_coords));
    noff.push_back((uint32_t)nb.size());
  }
  roff.assign(1, 0);
  for (uint32_t q = 0; q < n_ranges; q++) { rb += rnames[q]; roff.push_back((uint32_t)rb.size()); }
  auto up = [&](DevBuf &d, const void *src, size_t bytes) {
    d.reserve(std::max<size_t>(bytes, 256));
    if (bytes) IMPG_HIP(hipMemcpyAsync(d.p, src, bytes, hipMemcpyHostToDevice, s));
  };
  up(d_nb, nb.data(), nb.size()); up(d_noff, noff.data(), noff.size() * 4); up(d_shift, nshift.data(), nshift.size() * 4);
  up(d_rb, rb.data(), rb.size()); up(d_roff, roff.data(), roff.size() * 4);
  t = TextTables{d_nb.as<char>(), d_noff.as<uint32_t>(), d_shift.as<uint32_t>(), (uint32_t)ix.seq.names.size(), d_rb.as<char>(), d_roff.as<uint32_t>(),
                 nullptr, 0u};
  if (!with_lengths) return;
  // "--original-sequence-coordinates": no sequence files to ask, the lengths print as 0 (main.rs:12014-12046)
  for (const int64_t len : ix.seq.lens) lens.push_back(original_coords ? 0u : (uint32_t)len);
  up(d_len, lens.data(), lens.size() * 4);
  t.seq_len = d_len.as<uint32_t>();
  t.n_lens = (uint32_t)lens.size();
}

void device_text_pieces(Engine &E, const uint32_t *d_len, uint32_t n_rows, const char *what,
                        const std::function<void(uint32_t, uint32_t, const unsigned long long *, unsigned long long, char *)> &write,
                        const std::function<void(const char *, size_t)> &sink, std::atomic<uint64_t> &pieces, std::atomic<uint64_t> &bytes) {
  if (!n_rows) return;
  hipStream_t s = E.stream;
  DevBuf off, stmp;
  // ---- lengths -> 64-bit offsets (a transitive batch prints more than 4 GB) ----------------------------------------------
  off.reserve((size_t)(n_rows + 1) * 8);
  // piece boundaries: whole rows, at most PIECE bytes each; found on the host from a copy of the offsets
  const unsigned long long PIECE = (unsigned long long)E.opt.bed_text_piece_bytes;
  std::vector<unsigned long long> h_off(n_rows);
  const unsigned long long total = prims::offsets_and_total(stmp, d_len, off.as<unsigned long long>(), n_rows, s, h_off.data());
  const size_t cap = (size_t)std::min<unsigned long long>(total, PIECE) + 4096;
  // a piece holds whole rows; only a piece of one row can outgrow PIECE, and it must still fit the buffer.  Refused
  // here, with nothing queued and no pinned buffer in flight.
  for (uint32_t r = 0; r < n_rows; r++)
    if ((r + 1 < n_rows ? h_off[r + 1] : total) - h_off[r] > cap) throw Error{IMPG_E_UNSUPPORTED, std::string("a single ") + what + " row longer than the text buffer"};
  DevBuf piece[2];
  char *pin[2] = {nullptr, nullptr};
  struct Unpin { char **p; ~Unpin() { for (int k = 0; k < 2; k++) if (p[k]) (void)hipHostFree(p[k]); } } unpin{pin};
  for (int k = 0; k < 2; k++) { piece[k].reserve(cap); IMPG_HIP(hipHostMalloc((void **)&pin[k], cap, hipHostMallocDefault)); }
  hipEvent_t done[2];
  for (int k = 0; k < 2; k++) IMPG_HIP(hipEventCreateWithFlags(&done[k], hipEventDisableTiming));
  struct EvFree { hipEvent_t *e; ~EvFree() { (void)hipEventDestroy(e[0]); (void)hipEventDestroy(e[1]); } } evfree{done};
  struct Pending { size_t bytes; bool live; } pend[2] = {{0, false}, {0, false}};
  uint32_t r0 = 0;
  int slot = 0;
  while (r0 < n_rows || pend[0].live || pend[1].live) {
    if (r0 < n_rows) {
      // rows [r0, r1): as many whole rows as fit one piece
      const unsigned long long base = h_off[r0];
      uint32_t r1 = (uint32_t)(std::upper_bound(h_off.begin() + r0 + 1, h_off.end(), base + PIECE) - h_off.begin());
      if (r1 == n_rows) { if (total - base > PIECE && n_rows - 1 > r0) r1 = n_rows - 1; }
      else r1 = std::max(r1 - 1, r0 + 1);
      const unsigned long long end = r1 < n_rows ? h_off[r1] : total;
      write(r0, r1, off.as<unsigned long long>() + r0, base, piece[slot].as<char>());
      IMPG_HIP(hipMemcpyAsync(pin[slot], piece[slot].p, (size_t)(end - base), hipMemcpyDeviceToHost, s));
      IMPG_HIP(hipEventRecord(done[slot], s));
      pend[slot] = {(size_t)(end - base), true};
      pieces++;
      bytes += end - base;
      r0 = r1;
    }
    // consume the OTHER slot's piece while this one is in flight (or drain at the end)
    const int other = slot ^ 1;
    if (pend[other].live) {
      IMPG_HIP(hipEventSynchronize(done[other]));
      sink(pin[other], pend[other].bytes);
      pend[other].live = false;
    } else if (r0 >= n_rows && pend[slot].live) {
      IMPG_HIP(hipEventSynchronize(done[slot]));
      sink(pin[slot], pend[slot].bytes);
      pend[slot].live = false;
    }
    slot ^= 1;
  }
}

void TextStream::reserve(size_t bytes, hipStream_t s) {
  for (int k = 0; k < 2; k++)
    if (!done[k]) IMPG_HIP(hipEventCreateWithFlags(&done[k], hipEventDisableTiming));
  bytes = std::max<size_t>(bytes, 256);
  if (bytes <= cap) return;
  IMPG_HIP(hipStreamSynchronize(s));  // (nothing of an earlier text is in flight; said once more where buffers go away)
  for (int k = 0; k < 2; k++) {
    if (pin[k]) { (void)hipHostFree(pin[k]); pin[k] = nullptr; }
    cap = 0;
    piece[k].reserve(bytes);
    IMPG_HIP(hipHostMalloc((void **)&pin[k], bytes, hipHostMallocDefault));
  }
  cap = bytes;
  allocs++;
}

void TextStream::drop() {
  for (int k = 0; k < 2; k++) {
    if (pin[k]) (void)hipHostFree(pin[k]);
    if (done[k]) (void)hipEventDestroy(done[k]);
    pin[k] = nullptr;
    done[k] = nullptr;
    piece[k].release();
  }
  for (DevBuf *d : {&rows, &len, &off, &bad, &stmp}) d->release();
  tables.reset();
  cap = 0;
}

void device_text_windows(Engine &E, TextStream &S, const unsigned long long *h_off, uint32_t n_rec,
                         const std::function<void(uint32_t, uint32_t, unsigned long long, unsigned long long, char *)> &write,
                         const std::function<void(const char *, size_t)> &sink, std::atomic<uint64_t> &pieces, std::atomic<uint64_t> &bytes) {
  if (!n_rec) return;
  hipStream_t s = E.stream;
  const unsigned long long total = h_off[n_rec];
  const unsigned long long PIECE = std::max<unsigned long long>((unsigned long long)E.opt.bed_text_piece_bytes, 1);
  if (std::min(total, PIECE) > S.cap) throw Error{IMPG_E_INVALID, "internal: a text piece larger than the stream's buffers"};
  struct Pending { size_t bytes; bool live; } pend[2] = {{0, false}, {0, false}};
  // (a sink that throws leaves a copy in flight into a buffer the owner keeps: wait for it before anything else uses it)
  struct Settle { hipStream_t s; ~Settle() { (void)hipStreamSynchronize(s); } } settle{s};
  unsigned long long base = 0;
  uint32_t r0 = 0;  // the record that holds byte `base`
  int slot = 0;
  while (base < total || pend[0].live || pend[1].live) {
    if (base < total) {
      const unsigned long long n_bytes = std::min(PIECE, total - base), end = base + n_bytes;
      // records [r0, r1): r1 = the first record that starts at or behind the piece's end
      const uint32_t r1 = (uint32_t)(std::lower_bound(h_off + r0 + 1, h_off + n_rec, end) - h_off);
      write(r0, r1, base, n_bytes, S.piece[slot].as<char>());
      IMPG_HIP(hipMemcpyAsync(S.pin[slot], S.piece[slot].p, (size_t)n_bytes, hipMemcpyDeviceToHost, s));
      IMPG_HIP(hipEventRecord(S.done[slot], s));
      pend[slot] = {(size_t)n_bytes, true};
      pieces++;
      bytes += n_bytes;
      base = end;
      r0 = h_off[r1] == end ? r1 : r1 - 1;  // (r1 = n_rec at the text's end: nothing follows)
    }
    // consume the OTHER slot's piece while this one is in flight (or drain at the end)
    const int other = slot ^ 1;
    if (pend[other].live) {
      IMPG_HIP(hipEventSynchronize(S.done[other]));
      pend[other].live = false;
      sink(S.pin[other], pend[other].bytes);
    } else if (base >= total && pend[slot].live) {
      IMPG_HIP(hipEventSynchronize(S.done[slot]));
      pend[slot].live = false;
      sink(S.pin[slot], pend[slot].bytes);
    }
    slot ^= 1;
  }
}

}  // namespace impg
