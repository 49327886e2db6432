// read_parts.h — what the routes of preprocess.cpp and the share readers (share_reader.cpp, share_plan.h) have in common: the
// environment's switches, the owners of the parser's device blocks, and "finish a PackedReads and upload it".  Internal: no
// HIP in here, a host compiler takes it.
#pragma once
#include <stdlib.h>
#include <algorithm>
#include <string>
#include <utility>

#include "device_mem.h"
#include "fastq.h"
#include "fastq_gpu.h"

namespace shk {

const size_t FASTA_DEVICE_MIN_DEFAULT = (size_t)1 << 20;
const int DECLINED = 1;                 // what a route returns when the next one is to be tried (SHK_E_* are <= 0)

// the environment's switches, read once per call (the tests change them between handles of one process)
struct Knobs {
    static bool is(const char *v, char c) { return v && *v == c; }
    static uint64_t num(const char *v, uint64_t dflt) { return (v && *v) ? strtoull(v, nullptr, 10) : dflt; }
    const bool host_parser = is(getenv("SHK_HOST_PARSER"), '1'), gunzip_device = !is(getenv("SHK_GUNZIP_DEVICE"), '0');
    const size_t pipeline_min = num(getenv("SHK_FASTQ_PIPELINE_MIN"), 64ull << 20), stream_device_min = num(getenv("SHK_STREAM_DEVICE_MIN"), 8ull << 20);
    const size_t pieces = (size_t)std::max<long long>(1, (long long)num(getenv("SHK_FASTQ_PIECES"), 4));
    // FASTA texts below this many bytes go to the host packer (shk_preprocess_fasta; the default: DESIGN.md §5, profiles/fasta)
    const size_t fasta_device_min = num(getenv("SHK_FASTA_DEVICE_MIN"), FASTA_DEVICE_MIN_DEFAULT);
    // bases per batch of the host-parsed paths (a batch is limited to 2^32 packed bases by its 32-bit offsets)
    const uint64_t batch_bases = std::min<uint64_t>(std::max<uint64_t>(num(getenv("SHK_BATCH_BASES"), 1ull << 31), 1024), 3ull << 30);
    // text per window of route 2 (bytes; default 1 GiB — unmeasured so far): a window and its carry fit one batch.  Set: a BGZF
    // file beyond it takes route 2 even where it fits one batch.
    const BgzfWindowKnob window = bgzf_window_knob(2 * batch_bases);
};

// a device block of the parser that goes back to the pool when its owner goes out of scope (every error and
// "declined" exit), or at reset() where the success path lets go of it earlier
template <typename T, void (*Free)(T &)> struct Owned : T {
    Owned() = default;
    Owned(Owned &&o) noexcept : T(std::move(static_cast<T &>(o))) { static_cast<T &>(o) = T(); }
    Owned &operator=(Owned &&o) noexcept { if (this != &o) { reset(); T::operator=(std::move(o)); static_cast<T &>(o) = T(); } return *this; }
    ~Owned() { reset(); }
    void reset() { Free(*this); }
};
using Text = Owned<GpuText, gpu_text_free>;
using Packed = Owned<GpuPacked, gpu_packed_free>;

// the two arrays of a host-packed batch in HBM (device_upload: memory of their own, not the pool's), freed with their owner
struct DevPair { void *bases = nullptr, *seg_off = nullptr; };
inline void dev_pair_free(DevPair &p) { device_free(p.bases); device_free(p.seg_off); p = DevPair(); }
using UploadedReads = Owned<DevPair, dev_pair_free>;
// Finish a PackedReads and upload it.  Without a segment nothing is uploaded (`up` stays empty).  uploaded_bytes, where asked
// for, grows by the bytes of the two arrays.  0, or the code of device_upload (err: its text; nothing is held).
inline int upload_packed(PackedReads &pr, UploadedReads &up, std::string &err, uint64_t *uploaded_bytes = nullptr) {
    up.reset();
    if (pr.n_seg() == 0) return 0;
    pr.finish();
    int rc = device_upload(pr.bases.data(), pr.bases.size() * 4, &up.bases, err);
    if (!rc) rc = device_upload(pr.seg_off.data(), pr.seg_off.size() * 4, &up.seg_off, err);
    if (rc) { up.reset(); return rc; }
    if (uploaded_bytes) *uploaded_bytes += (pr.bases.size() + pr.seg_off.size()) * 4;
    return 0;
}

}  // namespace shk
