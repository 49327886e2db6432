// scan_gpu.h — what the device packers of fastq_gpu.hip and fasta_gpu.hip share: the exclusive scan and the grid size.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>

#include "device_mem.h"

namespace shk {

// blocks of `block` threads for `work` items, at least 1 and at most `cap`
static inline unsigned grid1(uint64_t work, unsigned block = 256, unsigned cap = 65536) {
    uint64_t b = (work + block - 1) / block; if (b < 1) b = 1; if (b > cap) b = cap; return (unsigned)b;
}

// In-place exclusive scan of a[0..n) on stream st; *d_total (device) receives the sum.  4096 items per workgroup and level
// (SCAN_ITEMS): more than that many items take a second level, more than 4096^2 a third.  0; -4; -5.  (fastq_gpu.hip)
static constexpr uint64_t SCAN_ITEMS = 4096;
int exclusive_scan(unsigned long long *a, uint64_t n, unsigned long long *d_total, hipStream_t st, PoolScope &sc, std::string &err);

}  // namespace shk
