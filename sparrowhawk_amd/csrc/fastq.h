// fastq.h — host FASTQ/gzip ingestion, quality masking, segmenting and 2-bit packing (SPEC S1-S2).
// Replaces the reader the reference's crate builds over web_sys::File + gz sniff + seq_io
// (/root/reference/AGENTS.md:180-183; sibling in tree: rust/orphos-bridge/src/fastx_wasm.rs:53-70).
#pragma once
#include "share_windows.h"
#include <stdint.h>
#include <stddef.h>
#include <functional>
#include <string>
#include <vector>
#include "bytebuf.h"

namespace shk {

struct PackedReads {
    std::vector<uint32_t> bases;     // 2-bit stream, base i in bits [2*(i%16)+1 : 2*(i%16)] of word i/16
    std::vector<uint32_t> seg_off;   // n_seg+1 base offsets
    uint64_t n_bases = 0;            // bases in the packed stream (valid segments >= k only)
    uint64_t n_reads = 0;            // FASTQ records seen
    uint64_t n_input_bases = 0;      // bases in the FASTQ records
    uint32_t cur = 0;                // partial word being filled
    void clear();
    void reset_stream();             // drop the packed stream (a batch was handed on), keep the read counters
    void finish();                   // flush the partial word, pad one spare word
    uint64_t n_seg() const { return seg_off.empty() ? 0 : seg_off.size() - 1; }
};

// progress(reads_so_far, bytes_consumed, bytes_total) is called every `every` reads (0 = never)
using ProgressFn = std::function<void(uint64_t, uint64_t, uint64_t)>;

// Appends the reads of one FASTQ buffer (plain or gzip) to `out`.  0 or SHK_E_PARSE(-3)/-4.
// flush(out) — optional — is called after a record when out.n_reads is a multiple of flush_reads (if non-zero)
// or the stream holds >= flush_bases bases: the caller takes the batch (PackedReads::finish + upload) and
// calls out.reset_stream().  Non-zero return aborts the parse with that code.
using FlushFn = std::function<int(PackedReads &)>;
int pack_fastq(const uint8_t *buf, size_t n, uint32_t k, uint32_t min_qual, PackedReads &out,
               std::string &err, uint64_t every = 0, const ProgressFn &progress = nullptr,
               uint64_t flush_reads = 0, uint64_t flush_bases = 0, const FlushFn &flush = nullptr,
               uint64_t rec_base = 0 /* records of this file that came before buf: numbering of the error messages */);

// The same for one FASTA buffer (plain or gzip; SPEC S1a): a record per header line, its lines joined, the maximal runs of
// ACGTacgt of the joined sequence as segments, a long run in pieces by the rule of pack_fastq.  There are no qualities.
// progress / flush: after a record, i.e. when the next header or the end of the text is met (bytes_consumed: where that
// header begins).  A non-blank line in front of the first header is -3, "FASTA: ..." (rec_base: records of this file that
// came before buf — a piece that begins at a header).  The device states the same rule in fasta_gpu.hip.
int pack_fasta(const uint8_t *buf, size_t n, uint32_t k, PackedReads &out, std::string &err, uint64_t every = 0,
               const ProgressFn &progress = nullptr, uint64_t flush_reads = 0, uint64_t flush_bases = 0,
               const FlushFn &flush = nullptr, uint64_t rec_base = 0);

// b[0..n) starts with a whole BGZF block (SAM spec 4.1: a gzip member with a 'BC' extra subfield that holds its size - 1):
// bsize = that size.  The one rule by which both the host reader and the device inflater (inflate_gpu.hip) walk a chain.
bool bgzf_block(const uint8_t *b, size_t n, size_t &bsize);
// A BGZF file as the host sees it before a byte crosses PCIe: every block's place, its ISIZE and CRC (they stand in its
// trailer), and — once cut — the windows of consecutive blocks whose text fits a budget (inflate_gpu.h: BgzfWindows).
struct BgzfChain {
    struct Block { uint64_t in_off; uint32_t bsize, hdr, isize, crc; };      // in_off: of the block's header in the file
    struct Window { size_t b0, b1; uint64_t in_off, in_end, text, text_before; uint32_t nonempty; };
    std::vector<Block> blocks;
    std::vector<Window> windows;
    uint64_t text = 0, nonempty = 0;      // bytes of text / non-empty blocks of the whole file
};
// Walks gz[0..n) as gpu_inflate_member walks a BGZF file (bgzf_block, FLG == 4, ISIZE <= 65536, empty blocks checked by zlib).
// 0: out.blocks, out.text, out.nonempty are set; 1: not a complete chain of such blocks, or smaller than SHK_GUNZIP_DEVICE_MIN
// (*why).
int bgzf_walk(const uint8_t *gz, size_t n, BgzfChain &out, const char *&why);
// out.windows from out.blocks; -1: a block exceeds the budget
int bgzf_cut_windows(BgzfChain &c, uint64_t budget);
// SHK_GUNZIP_DEVICE_WINDOW, bytes of text per window: 1 GiB by default, at most max_bytes (a window and its carry fit one
// batch) and 3 GiB (32-bit offsets), at least one block of 64 KiB
struct BgzfWindowKnob { bool set; uint64_t bytes; };
BgzfWindowKnob bgzf_window_knob(uint64_t max_bytes);
// bytes of a FASTQ text without its trailing blank lines: what gpu_upload_text (fastq_gpu.h) uploads of t[0..n)
size_t trimmed_len(const uint8_t *t, size_t n);
// (the windows of a BGZF chain and the ranks' runs of its blocks — plan_bgzf_windows, plan_fastq_slices, plan_share_windows —
// and slice_cut: share_windows.h, which a host compiler takes alone)
// Where the last FASTQ record of t[0..n) starts that is known to be one: a line that begins with '@' and whose line after
// next begins with '+' (the rule of next_record_start in preprocess.cpp; a quality line may begin with '@', but its line
// after next is a sequence).  A line whose line after next has not begun inside t is undecided and is passed over.  Byte 0
// begins a line.  UINT64_MAX: no such line.  The device states the same rule in k_last_record_start (inflate_gpu.hip).
uint64_t last_record_start(const uint8_t *t, size_t n);
// The same rule read forwards — where the slices of the sharded FASTQ entry point are cut: the smallest p >= from that
// begins a line (p == 0 or t[p - 1] == '\n'), holds '@', and whose line after next begins with '+'.  A line whose line
// after next has not begun inside t is undecided: the search stops there and never passes it over (a caller that sees only
// a part of the text widens its view and asks again; two callers with different views of one text so arrive at the same
// start).  UINT64_MAX: none, or undecided.  The device states the same rule in k_first_record_start (inflate_gpu.hip).
uint64_t first_record_start(const uint8_t *t, size_t n, size_t from);
// Slice `rank` of `world` of the text t[0..e) (e: without its trailing blank lines), [s0, s1): s_0 = 0, s_world = e, and in
// between s_r = the first record start at or after the nominal cut c_r (e where there is none).  cut0 / cut1: c_rank and
// c_(rank + 1) — floor(r * e / world) for plain text and the text of a plain gzip member (slice_cut), for a BGZF chain the
// text offset at which block first_block[r] of plan_fastq_slices begins.
void fastq_slice_bounds(const uint8_t *t, size_t e, uint32_t rank, uint32_t world, uint64_t cut0, uint64_t cut1, uint64_t &s0, uint64_t &s1);
// FASTA (RecFmt::Fasta, share_windows.h; SPEC S1a): a record starts at p when t[p] == '>' and p begins a line (p == 0 or t[p - 1] == '\n'; a lone '\r' ends
// no line).  A line is decided by its own first byte, so a partial view leaves nothing open but whether its first byte begins
// a line.  first: the smallest such p >= from; last: the largest such p < n; UINT64_MAX: none.  The device states the same rule
// in k_fasta_header_search (inflate_gpu.hip).
uint64_t fasta_first_record_start(const uint8_t *t, size_t n, size_t from);
uint64_t fasta_last_record_start(const uint8_t *t, size_t n);
// the twin of fastq_slice_bounds: s_0 = 0, s_world = e, in between s_r = the first FASTA record start at or after c_r (e where
// there is none).  Slices may be empty; a non-blank line in front of the file's first header lies in slice 0.
void fasta_slice_bounds(const uint8_t *t, size_t e, uint32_t rank, uint32_t world, uint64_t cut0, uint64_t cut1, uint64_t &s0, uint64_t &s1);
// gzip sniff (1F 8B) + multi-member inflate; plain input is passed through (p/n point at buf or at `storage`)
int maybe_inflate(const uint8_t *buf, size_t n, ByteVec &storage, const uint8_t *&p, size_t &pn,
                  std::string &err);
// the two files of a pair in two threads (b2 may be null); BGZF input is inflated block-parallel either way
int maybe_inflate_pair(const uint8_t *b1, size_t n1, const uint8_t *b2, size_t n2, ByteVec &s1,
                       ByteVec &s2, const uint8_t *&p1, size_t &l1, const uint8_t *&p2, size_t &l2,
                       std::string &err);

}  // namespace shk
