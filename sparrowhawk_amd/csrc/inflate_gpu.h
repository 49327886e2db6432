// inflate_gpu.h — one gzip member, or one BGZF (bgzip) file, inflated ON THE DEVICE (inflate_gpu.hip): the compressed bytes
// are what crosses PCIe, the FASTQ text is born in HBM and goes straight to the device parser (fastq_gpu.h).  A plain
// member: the same two-pass scheme as the host reader (inflate_mt.cpp, after pugz / rapidgzip) with thousands of chunks
// instead of one per host thread.  A BGZF file: one wave per block, no speculation (every block is a stream of its own).
// A BGZF file of more text than is inflated at once goes window by window (BgzfWindows below): the same inflater on a run of
// blocks at a time (inflate_gpu.hip: inflate_block_run, the one launch of the two kernels), k_last_record_start to cut the
// window's text where its last whole record ends, and the one end-of-text rule (trim_text_end) for the last window.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string>
#include <thread>
#include <vector>
#include "device_mem.h"
#include "fastq.h"
#include "fastq_gpu.h"
#include "share_windows.h"

namespace shk {

struct GpuInflateStats {
    double h2d_ms = 0, search_ms = 0, decode_ms = 0, windows_ms = 0, resolve_ms = 0, total_ms = 0;
    uint64_t chunks = 0, text_bytes = 0;
    uint64_t blocks = 0;                 // a BGZF file: its non-empty blocks, one wave each (search_ms and windows_ms stay 0)
    const char *why_not = "";            // when the member was not taken: the reason (for the logs and the tests)
};

// gz[0..n): ONE plain gzip member (nothing behind its trailer) of FASTQ-like text, or a BGZF file: a chain of BGZF blocks
// from the first byte to the last (empty blocks anywhere, the end-of-file block or none; any data).  Returns
//   0  the text is on `device` in out (a GpuText as gpu_upload_text makes them: trailing blank lines cut, 32 zero bytes
//      behind it); the bytes are exactly what zlib would produce — CRC-32 and ISIZE of the trailer verified;
//   1  not taken: too small, several members, stored / binary data, no block starts found, a chunk that does not end where
//      the next begins, more output than the room, a checksum that does not match; a BGZF file: smaller than
//      SHK_GUNZIP_DEVICE_MIN, a chain that does not cover the file, a block whose stream is damaged, does not give exactly
//      ISIZE bytes or does not end in its last byte, out of device memory — the caller inflates on the host (which also
//      owns the error messages of a damaged stream);
//  <0  -4 out of device memory (a plain member), -5 HIP error.
// raw: every byte of the member stays as it is (out.e = the member's size; the tests compare with zlib) — otherwise the text
// is made ready for the parser (trailing blank lines cut, see above).
// walked: the file's chain as bgzf_walk (fastq.h) has walked it already, or null
int gpu_inflate_member(const uint8_t *gz, size_t n, int device, void *stream, GpuText &out, std::string &err,
                       GpuInflateStats *stats = nullptr, bool raw = false, const BgzfChain *walked = nullptr);

// ---- a BGZF file of any size, window by window ------------------------------------------------------------------------
// The chain is walked on the host before a byte crosses PCIe (every block's ISIZE stands in its trailer), cut into windows
// of consecutive blocks whose text fits a budget (fastq.h: BgzfChain, bgzf_walk, bgzf_cut_windows, the budget: bgzf_window_knob
// — host code, declared there), and each window is uploaded, inflated with window-relative descriptors, and cut at its last
// record start on the device (BgzfWindows::step).

// The device side of one file's windows: two input buffers (window w + 1 is uploaded, from a helper thread, while window w
// is worked on) and two text buffers (window w's text starts with the carry: the partial record left over from window w - 1).
//     if (bw.open(gz, &chain, device, stream, err)) ...
//     for (size_t w = 0; w < chain.windows.size(); w++) { if (bw.step(w, raw, carry, cut, unterminated, why, err)) ...; use text(w)[0..cut) }
class BgzfWindows {
  public:
    static const uint64_t CARRY_MAX = 16ull << 20;        // a partial record of more than this goes to the host reader
    BgzfWindows() = default;
    ~BgzfWindows() { close(); }
    BgzfWindows(const BgzfWindows &) = delete;
    BgzfWindows &operator=(const BgzfWindows &) = delete;
    // 0; 1 out of device memory (nothing is held); -5
    int open(const uint8_t *gz, const BgzfChain *chain, int device, void *stream, std::string &err);
    void close();                                         // the helper thread is joined, then the blocks go back
    // Windows in order, w = 0, 1, ...: window w is inflated behind `carry` bytes at the front of text(w) while window w + 1
    // is uploaded.  Not the last window: cut = its last record start (k_last_record_start), text(w)[cut..) goes to the front
    // of text(w + 1) and is the new carry, 32 zero bytes follow text(w)[0..cut) as the parser wants them.  The last window:
    // cut = its end without trailing blank lines (the rule of gpu_upload_text), zero bytes as before, the new carry is 0.
    // raw: the bytes stay as they are — the last window is not trimmed, and a window without a usable record start is handed
    // on whole (cut = its end).
    // 0; 1: this window is the host reader's (*why: a damaged block, more to carry than CARRY_MAX, kilobytes of blank lines
    // at the end), carry is as it was; -5
    int step(size_t w, bool raw, uint64_t &carry, uint64_t &cut, bool &unterminated, const char *&why, std::string &err);
    uint8_t *text(size_t w) const { return (uint8_t *)d_text_[w & 1].p; }
    double h2d_ms = 0, decode_ms = 0;                      // summed over the windows
    uint64_t uploaded = 0;                                 // compressed bytes of the windows worked on so far
    // The parts step() is made of, for a caller that cuts its windows elsewhere (BgzfShareWindows below: a rank's run begins
    // and ends inside a window).  inflate: window w behind `carry` bytes in text(w), n = carry + its text; window w + 1 is sent
    // ahead where asked for (a window nobody sent ahead travels when its turn comes).  first_start / last_start: the record
    // starts of text(w)[0..n) by the kernels' rules (UINT64_MAX: none / undecided).  trim_end: the end-of-text rule on
    // text(w)[0..n).  carry_on: text(w)[cut..n) to the front of text(w + 1), 32 zero bytes behind the cut.
    // Each 0; 1 (*why) where step() returns 1; -5.
    int inflate(size_t w, bool prefetch_next, uint64_t carry, uint64_t &n, const char *&why, std::string &err);
    int first_start(size_t w, uint64_t n, uint64_t from, uint64_t &at, std::string &err, RecFmt fmt = RecFmt::Fastq);
    int last_start(size_t w, uint64_t n, uint64_t &at, std::string &err, RecFmt fmt = RecFmt::Fastq);
    int trim_end(size_t w, uint64_t n, uint64_t &e, bool &unterminated, const char *&why, std::string &err);
    int carry_on(size_t w, uint64_t n, uint64_t cut, std::string &err);
    void *stream() const { return st_; }
  private:
    void upload(size_t w);                                // blocking, on a stream of its own: -> up_[w & 1]
    size_t up_w_[2] = {SIZE_MAX, SIZE_MAX};                // the window whose bytes d_in_[i] holds
    const uint8_t *gz_ = nullptr; const BgzfChain *chain_ = nullptr;
    int device_ = 0; void *st_ = nullptr;
    PoolBlock d_in_[2], d_text_[2], d_desc_, d_status_, d_bad_;
    struct Upload { int rc = 0; std::string err; double ms = 0; } up_[2];
    std::thread prefetch_;                                // uploads window w + 1 during step(w); joined by step(w + 1) and close()
};

// One rank's run of a walked BGZF chain, of any size, window by window: the slice gpu_bgzf_slice hands over in one piece, in
// pieces of whole records.  The run (fastq.h: plan_fastq_slices) is cut into windows of at most `budget` bytes of text
// (share_windows.h: plan_share_windows); the non-empty block in front of the run rides with window 0 (k_first_record_start
// finds s_rank there), every window but the last is cut at its last record start and the rest is carried (BgzfWindows), and
// s_(rank + 1) is looked for in small windows of follow-on blocks of run rank + 1 — 2 non-empty blocks, then twice as many
// while it is undecided, up to BgzfWindows::CARRY_MAX of text.  Window w + 1 is uploaded while the caller works on window w;
// only the rank's blocks and these few neighbours cross PCIe.
//     if (sw.open(gz, chain, rank, world, budget, device, stream, why, err)) ...          // 1: declined, nothing was uploaded
//     for (;;) { if (sw.next(piece, at, done, why, err)) ...; if (done) break; parse piece; }
// A piece is text in the parser's form (16-byte aligned, 32 zero bytes behind) that stays the object's: it is good until the
// next call.  at: where the piece begins in the file's text.  next() returns 1 (*why) where a window is the host reader's: the
// host reads the file, cuts the same slice and goes on at consumed() (everything in front of it has been handed over).
class BgzfShareWindows {
  public:
    BgzfShareWindows() = default;
    ~BgzfShareWindows() { close(); }
    BgzfShareWindows(const BgzfShareWindows &) = delete;
    BgzfShareWindows &operator=(const BgzfShareWindows &) = delete;
    int open(const uint8_t *gz, const BgzfChain &chain, uint32_t rank, uint32_t world, uint64_t budget, int device, void *stream,
             const char *&why, std::string &err, RecFmt fmt = RecFmt::Fastq);
    int next(GpuText &piece, uint64_t &at, bool &done, const char *&why, std::string &err);
    void close();
    uint64_t run_text() const { return c1_ - c0_; }        // bytes of text of the rank's run (the sum of its ISIZE fields)
    uint64_t run_begin() const { return c0_; }
    uint64_t consumed() const { return consumed_; }        // the file's text in front of this offset is done with
    uint64_t uploaded() const { return bw_.uploaded; }
    uint64_t windows() const { return windows_; }          // windows inflated so far
    double h2d_ms() const { return bw_.h2d_ms; }
    double decode_ms() const { return bw_.decode_ms; }
  private:
    BgzfChain view_;                                       // the chain's blocks with the windows of THIS rank
    BgzfWindows bw_;
    PoolBlock first_;                                      // a piece that does not begin where its window's buffer begins
    size_t B_ = 0, n_own_ = 0, w_ = 0;
    uint32_t rank_ = 0;
    RecFmt fmt_ = RecFmt::Fastq;                           // the format its windows and its slice are cut by
    uint64_t c0_ = 0, c1_ = 0, carry_ = 0, consumed_ = 0, windows_ = 0;
    bool started_ = false, done_ = false;
};

// k_last_record_start alone on n bytes of host text (the tests compare it with last_record_start)
int gpu_last_record_start(const uint8_t *t, size_t n, int device, uint64_t &at, std::string &err);
// its forward twin, k_first_record_start, alone (the tests compare it with first_record_start); at = UINT64_MAX: none / undecided
int gpu_first_record_start(const uint8_t *t, size_t n, uint64_t from, int device, uint64_t &at, std::string &err);

// k_fasta_header_search alone on n bytes of host text (the tests compare it with fasta_first_record_start / fasta_last_record_start;
// last: `from` is not used)
int gpu_fasta_record_start(const uint8_t *t, size_t n, bool last, uint64_t from, int device, uint64_t &at, std::string &err);

// ---- one rank's slice of a file, for the sharded FASTQ and FASTA entry points (share_reader.cpp: read_fastq_share) ---------
// The slice rule is stated in fastq.h (first_record_start, fastq_slice_bounds, plan_fastq_slices; FASTA: fasta_first_record_start,
// fasta_slice_bounds); here it is applied to text that is born on the device.  fmt: the record format the cuts go by (FASTQ where
// nothing is said: k_first_record_start / k_last_record_start; FASTA: k_fasta_header_search).  A span is a run of text inside a
// device block it owns.
struct DevSpan { PoolBlock blk; uint64_t off = 0, len = 0; bool unterminated = false; };
// A walked BGZF chain: rank r uploads and inflates the blocks of run r only (plan_fastq_slices), the non-empty block in front
// of the run (whether the run's first byte begins a line is written there) and the follow-on blocks of run r + 1 in which its
// slice ends — 2 first, then twice as many while the boundary is undecided, up to BgzfWindows::CARRY_MAX of text — with
// inflate_block_run, and finds s_r and s_(r + 1) with k_first_record_start.  uploaded: the compressed bytes that crossed PCIe.
// 0: out is the slice (possibly empty); 1: declined (*why: a damaged block, no boundary within reach, out of device memory) —
// the caller reads the file on the host and cuts the same slice there; -5.
int gpu_bgzf_slice(const uint8_t *gz, const BgzfChain &chain, uint32_t rank, uint32_t world, int device, void *stream, DevSpan &out,
                   uint64_t &uploaded, const char *&why, std::string &err, RecFmt fmt = RecFmt::Fastq);
// A whole text on the device (a plain gzip member inflated by gpu_inflate_member; nominal cuts floor(r * e / world)): its
// block becomes the span's.  0; -4; -5.
int gpu_text_slice(GpuText &text, uint32_t rank, uint32_t world, void *stream, DevSpan &out, std::string &err, RecFmt fmt = RecFmt::Fastq);
// A piece of a span for the parser, where the span is more than one batch takes: span text [from, from + want) cut back to
// its last record start — or all that is left, where that is no more than `want` — copied into a text of its own (16-byte
// aligned, 32 zero bytes behind).  next: where the following piece begins (span.len: this was the last; out.e == 0: nothing was
// left).  0; 1: no record starts inside the piece (not regular FASTQ: the host parser's; FASTA: one record beyond `want`, which
// ends at span offset `next`); -4; -5.
int gpu_span_piece(const DevSpan &span, uint64_t from, uint64_t want, void *stream, GpuText &out, uint64_t &next, std::string &err,
                   RecFmt fmt = RecFmt::Fastq);
// The spans back to back in one text as the parser wants it (16-byte aligned start, 32 zero bytes behind, a newline between
// two files where the first ends without one).  0; -4; -5.
int gpu_join_spans(const DevSpan *spans, int n_spans, void *stream, GpuText &out, std::string &err);

}  // namespace shk
