// share_reader.h — one rank's share of FASTQ files as packed batches in HBM (share_reader.cpp; routes 8 and 9 of preprocess.cpp's
// table): what shk_shard_preprocess_fastq hands to the shard layer and (a share of one batch) shk_device_pack_fastq_slice copies
// back.  Slice `rank` of `world` of every file (fastq.h: the slice rule; world 1: the whole file).  Routes, per file: a BGZF
// chain — the blocks of the rank's run alone are uploaded and inflated (inflate_gpu.h: gpu_bgzf_slice, BgzfShareWindows); a
// plain gzip member — inflated whole on the device, then cut (a deflate stream cannot be entered in the middle); plain text —
// cut on the host, the slice alone is uploaded.  Whatever the device declines is read on the host, whole, and cut there by the
// same rule; text that is not regular 4-line FASTQ goes through the host parser, which owns the messages (record numbers count
// from the slice's start).  What the host decides beforehand — the kind of each file, the cuts, the text of the share — is
// share_plan.h's.
//   A share that fits ONE batch (SHK_BATCH_BASES): read_fastq_share — both files of a pair pooled into the one batch.
//   A larger one (the sharded entry point alone): read_fastq_share says so (in_batches) before it uploads anything, where the
//   ISIZE sums of the rank's run or the slice bounds of plain text tell, and read_fastq_share_batches then hands the share to
//   pass 1 batch by batch: a BGZF run in windows of at most SHK_GUNZIP_DEVICE_WINDOW of text, everything else in pieces of about
//   2 * SHK_BATCH_BASES bytes cut at record starts; the files of a pair one after the other.
// The same two readers serve shk_shard_preprocess_fasta (fmt = RecFmt::Fasta; SPEC S1a, the slice rule): the bounds are header
// lines, the packers are gpu_pack_fasta / pack_fasta, a byte of text is a base (pieces of at most SHK_BATCH_BASES bytes), a single
// record beyond one batch is SHK_E_PARAM, and the files of a pair are packed separately (one batch per file).
#pragma once
#include <string>
#include <vector>

#include "read_parts.h"
#include "share_windows.h"

struct FastqShare {
    // A share that fits one batch is held as batches: FASTQ — the one pooled batch of the file or the pair; FASTA — one per file
    // (the packers' rule on the lines in front of the first header holds per file).  A batch lies in the blocks of the device
    // parser or in a host-packed upload; either owner frees itself.
    struct Batch {
        shk::Packed gp; shk::UploadedReads up;
        uint64_t n_seg = 0, n_bases = 0, n_reads = 0;
        const uint32_t *d_bases() const { return gp.d_bases ? gp.d_bases : (const uint32_t *)up.bases; }      // (null: the host packer found no segment)
        const uint32_t *d_seg_off() const { return gp.d_seg_off ? gp.d_seg_off : (const uint32_t *)up.seg_off; }
    };
    std::vector<Batch> batches;
    uint64_t n_seg = 0, n_bases = 0, n_reads = 0, n_input_bases = 0;      // summed over the batches (in_batches: over those handed on)
    uint64_t uploaded_bytes = 0;                          // compressed or text (or host-packed) bytes that crossed PCIe
    uint32_t n_bgzf_slice = 0, n_member_whole = 0, n_text_slice = 0, n_host = 0;      // files by route; n_host: read or parsed on the host
    std::string route;                                    // the routes' names, '+' between two that differ
    bool in_batches = false;                              // the share exceeds one batch: nothing is held, read_fastq_share_batches reads it
    uint64_t text_ub = 0;                                 // in_batches: bytes of text of the share, or an upper bound (text_ub / 2 bounds its k-mer instances)
    uint64_t n_batches = 0, n_windows = 0;                // batches handed to pass 1; windows and pieces of text they were parsed from
    FastqShare() = default;
    FastqShare(const FastqShare &) = delete;
    FastqShare &operator=(const FastqShare &) = delete;
};
// SHK_OK, or the SHK_E_* code with its message in err; an oversized share (beyond one batch) is SHK_E_PARAM unless
// allow_batches (then SHK_OK with out.in_batches)
// fmt: the record format — the slice bounds, the packers (FASTA: gpu_pack_fasta from SHK_FASTA_DEVICE_MIN bytes of host-resident
// slice on, pack_fasta below it; text born on the device is packed there), the cut of pieces and the bases per byte of text
int read_fastq_share(const uint8_t *fq1, size_t n1, const uint8_t *fq2, size_t n2, uint32_t k, uint32_t min_qual, uint32_t rank,
                     uint32_t world, int device, void *stream, FastqShare &out, std::string &err, bool allow_batches = false,
                     shk::RecFmt fmt = shk::RecFmt::Fastq);

// where the batches of a share go: pass 1 of the shard layer (shard_preprocess.cpp: sp_pass1, the Sink)
struct ShardBatchSink {
    virtual ~ShardBatchSink() = default;
    // One batch (< 2^32 bases; n_seg == 0: reads without a segment) -> pass 1; the batch's memory is the caller's again on return.
    // reads: this rank's reads so far, the batch's included; text_done of text_total: how much of the share's text is consumed
    // (the percentage of the progress string).  SHK_OK, or the code of an error that is set in the handle.
    virtual int batch(const uint32_t *d_bases, const uint32_t *d_seg_off, uint64_t n_seg, uint64_t n_bases, uint64_t reads,
                      uint64_t text_done, uint64_t text_total) = 0;
};
// The share of any size, batch by batch into `sink`; out: the counters (nothing is held).  SHK_OK; the SHK_E_* code of a reading
// error with its message in err; or the code sink.batch returned, with err empty.
int read_fastq_share_batches(const uint8_t *fq1, size_t n1, const uint8_t *fq2, size_t n2, uint32_t k, uint32_t min_qual, uint32_t rank,
                             uint32_t world, int device, void *stream, ShardBatchSink &sink, FastqShare &out, std::string &err,
                             shk::RecFmt fmt = shk::RecFmt::Fastq);
