// bgzf_write_gpu.h — text in HBM written as a finished BGZF file on the device (bgzf_write_gpu.hip; SPEC S11a): the
// counterpart of inflate_gpu.h's k_bgzf_decode.  One wave per block of 65 280 bytes encodes it with the block encoder the
// host shares (deflate_write.h), a scan of the block sizes and one gather kernel lay the blocks back to back with their
// headers, trailers and the end marker, and the file is all that is downloaded.  Text that is still JSON-escaped (the fields
// of get_assembly()) is unescaped first, by a stream compaction.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <functional>
#include <string>
#include <vector>

#include "device_mem.h"

namespace shk {

struct BgzfWriteStats { double kernels_ms = 0, d2h_ms = 0; uint64_t text_bytes = 0, file_bytes = 0, blocks = 0, stored_blocks = 0; };

// chunk of the unescape kernels: one workgroup of 256 threads, 8 consecutive bytes a thread (the tests put escape pairs on
// both kinds of boundary)
static constexpr uint32_t UNESC_CHUNK = 2048, UNESC_PER_THREAD = 8;

// d_src[0..n) on the current device, readable on `stream`; escaped: JSON string content whose escapes (\n \t \" \\) are
// undone first.  file := the BGZF file, file_n bytes of it, in pinned host memory.  wait: waits for the stream (null:
// hipStreamSynchronize); timers: the kernels are timed with events (kernels_ms).  Device memory comes from the pool.
// 0; -1 a text beyond the kernels' counters; -4 out of device memory; -5 HIP error; -6 the text holds a backslash that begins
// none of the four escapes, or a block did not come out at the size its plan gave.
#ifdef __HIPCC__
int gpu_bgzf_write_pinned(const uint8_t *d_src, uint64_t n, bool escaped, void *stream, bool timers, const std::function<int(std::string &)> *wait,
                          PinnedBuf &file, size_t &file_n, BgzfWriteStats &S, std::string &err);
// the same from host memory (uploaded first)
int gpu_bgzf_write_host_pinned(const uint8_t *src, uint64_t n, bool escaped, void *stream, bool timers, const std::function<int(std::string &)> *wait,
                               PinnedBuf &file, size_t &file_n, BgzfWriteStats &S, std::string &err);
#endif
// from host memory into host memory, on the current device's null stream (shk_device_bgzf_compress)
int gpu_bgzf_write_host(const uint8_t *src, uint64_t n, bool escaped, bool timers, std::vector<uint8_t> &file, BgzfWriteStats &S, std::string &err);

}  // namespace shk
