// fasta_gpu.h — device-side FASTA packer (fasta_gpu.hip); the packed layout of fastq.h and fastq_gpu.h.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string>

#include "fastq_gpu.h"

namespace shk {

// text bytes per workgroup of the packer's kernels: the header state at a chunk's first byte comes from a carry over the chunks
// in front of it, and the counts of all chunks go through exclusive_scan (4096 per level: a second level beyond 16 MiB of text)
static constexpr uint32_t FASTA_GPU_CHUNK = 4096;

// t1/t2: plain FASTA texts in host memory (t2 may be null; a newline is supplied between them where t1 lacks its last one),
// or `uploaded`: one text that lies on the device already (t2 must be null).  SPEC S1a, byte-parallel: records of any length.
// Returns 0 = packed on the device (out as gpu_pack_fastq fills it: (n_bases >> 4) + 2 words, zero behind the last base;
// progress_bytes: one entry per `every` records, the offset at which the next record begins, bit 63 = second file),
// 1 = declined — a non-blank line in front of the first header of a file, or more than a batch holds (2^32 bases): the caller
// runs the host packer, which owns the messages — < 0 = error (-4 memory, -5 HIP, -1 a bad argument).
// read_base: records that came before this text (earlier pieces of the same input, each beginning at a header).
int gpu_pack_fasta(const uint8_t *t1, size_t n1, const uint8_t *t2, size_t n2, uint32_t k, uint64_t every, void *stream,
                   GpuPacked &out, std::string &err, uint64_t read_base = 0, const GpuText *uploaded = nullptr);

}  // namespace shk
