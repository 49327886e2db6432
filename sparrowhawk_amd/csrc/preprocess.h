// preprocess.h — how reads reach the counting passes (preprocess.cpp): the bodies of the preprocess entry points
// of the C ABI.  api.cpp runs each of them under guarded().
#pragma once
#include "handle.h"
#include "fastq_gpu.h"
#include "share_reader.h"      // routes 8 and 9: one rank's share of FASTQ / FASTA files
#include "share_windows.h"

int preprocess_impl(shk_handle *h, const uint8_t *fq1, size_t n1, const uint8_t *fq2, size_t n2);
// shk_preprocess_fasta: whole FASTA files, plain or gzip (SPEC S1a), by the device packer (fasta_gpu.h) or the host packer
int preprocess_fasta_impl(shk_handle *h, const uint8_t *fa1, size_t n1, const uint8_t *fa2, size_t n2);
int push_reads_impl(shk_handle *h, const uint8_t *chunk, size_t n);
int finish_reads_impl(shk_handle *h);
int preprocess_packed_device_impl(shk_handle *h, const void *d_bases, const void *d_seg_off, uint64_t n_seg,
                                  uint64_t n_bases, uint64_t n_reads);
int preprocess_packed_host_impl(shk_handle *h, const uint32_t *bases, const uint32_t *seg_off, uint64_t n_seg,
                                uint64_t n_bases, uint64_t n_reads);
// the count below which pass 2 emits no row (the shard layer's pass 2 uses the same)
uint32_t emit_threshold_of(const shk_handle *h);
