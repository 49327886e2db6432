// shard_preprocess.h — the sharded preprocess (shard_preprocess.cpp; DESIGN.md "Multi-GPU"): the bodies of the shk_shard_*
// entry points of the C ABI.  api.cpp runs each of them under guarded().
#pragma once
#include "handle.h"
#include "share_windows.h"     // RecFmt

struct shk_comm { shk::ShardComm *c = nullptr; };

// the collective calls: one packed batch in HBM, several, or the rank's share of FASTQ / FASTA files.  A collective that failed
// on this rank alone has aborted the communicator when they return (the peers' waits end: shard_comm.h, comm_stream_wait).
int shard_preprocess_one_impl(shk_handle *h, shk_comm *cm, const void *d_bases, const void *d_seg_off, uint64_t n_seg, uint64_t n_bases,
                              uint64_t n_reads, uint32_t n_partitions);
int shard_preprocess_batches_impl(shk_handle *h, shk_comm *cm, uint32_t n_batches, const void *const *d_bases, const void *const *d_seg_off,
                                  const uint64_t *n_seg, const uint64_t *n_bases, uint64_t n_reads, uint32_t n_partitions);
int shard_preprocess_fastq_impl(shk_handle *h, shk_comm *cm, const uint8_t *fq1, size_t n1, const uint8_t *fq2, size_t n2,
                                uint32_t n_partitions, int split, shk::RecFmt fmt);

// the single-GPU preprocess cut at its two exchange points: the steps a caller with collectives of its own drives
// (sparrowhawk_amd/dist.py), and which the collective calls above run between theirs
int shard_partition_impl(shk_handle *h, const void *d_bases, const void *d_seg_off, uint64_t n_seg, uint64_t n_bases,
                         uint64_t n_reads, uint32_t n_partitions, uint64_t *part_records);
int shard_pack_impl(shk_handle *h, void *d_send, const uint64_t *base_records, uint32_t n_partitions);
int shard_count_impl(shk_handle *h, const void *d_recv, const uint64_t *run_off, const uint32_t *run_cnt, uint32_t n_owned,
                     uint32_t n_sources, uint64_t *histo500_local, uint64_t *n_instances_local,
                     const void *d_recv_w = nullptr /* weights of the records (deduplicated by their sources) */);
int shard_rows_impl(shk_handle *h, const uint64_t *histo500_global, const void **d_keys, const void **d_cnt, uint64_t *n_rows,
                    uint32_t *used_min_count);
int shard_set_solid_impl(shk_handle *h, const void *const *d_keys, const void *d_cnt, uint64_t n_rows, uint64_t n_instances_global);
