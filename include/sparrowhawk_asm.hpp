// sparrowhawk_asm.hpp — header-only C++ mirror of the reference's AssemblyHelper
// (/root/reference/www/src/workers/Assembler.ts:15-39) over the C ABI in shk.h.  Same five
// members, same argument order; throws std::runtime_error where the Rust crate panics
// (Assembler.ts:93-106 catches that as a JS exception).  The stage-level helpers of shk.h — the host-only
// shk_host_* self tests, shk_device_gunzip, shk_device_unitig_assemble — have no counterpart in the
// reference's interface and are not mirrored here: call them through shk.h.
#pragma once
#include <stdexcept>
#include <string>
#include <vector>
#include "shk.h"

namespace sparrowhawk {

class AssemblyHelper {
public:
    // AssemblyHelper::new — a static factory in the reference, not a constructor (Assembler.ts:94)
    static AssemblyHelper new_(uint32_t k, bool verbose, uint32_t min_count, uint32_t min_qual,
                               uint64_t chunk_size, bool do_bloom, bool do_fit,
                               bool no_bubble_collapse, bool no_dead_end_removal) {
        shk_handle *h = shk_new(k, verbose, min_count, min_qual, chunk_size, do_bloom, do_fit,
                                no_bubble_collapse, no_dead_end_removal);
        if (!h) throw std::runtime_error(shk_new_error_message());
        return AssemblyHelper(h);
    }
    AssemblyHelper(AssemblyHelper &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    AssemblyHelper(const AssemblyHelper &) = delete;
    AssemblyHelper &operator=(const AssemblyHelper &) = delete;
    ~AssemblyHelper() { shk_free(h_); }

    void preprocess(const std::vector<uint8_t> &file1, const std::vector<uint8_t> *file2 = nullptr) {
        check(shk_preprocess(h_, file1.data(), file1.size(), file2 ? file2->data() : nullptr,
                             file2 ? file2->size() : 0));
    }
    // the same for FASTA files, plain or gzip (shk.h: shk_preprocess_fasta; SPEC S1a)
    void preprocess_fasta(const std::vector<uint8_t> &file1, const std::vector<uint8_t> *file2 = nullptr) {
        check(shk_preprocess_fasta(h_, file1.data(), file1.size(), file2 ? file2->data() : nullptr,
                                   file2 ? file2->size() : 0));
    }
    // preprocess(file1, file2 | null) across the ranks of a communicator (shk.h: shk_shard_preprocess_fastq; collective, and
    // so is assemble() after it).  split: every rank passes the same file(s) and takes its slice; otherwise the files are
    // this rank's own reads (file1 == nullptr: it has none).
    void sharded_preprocess_fastq(shk_comm *comm, const std::vector<uint8_t> *file1, const std::vector<uint8_t> *file2 = nullptr,
                                  bool split = true, uint32_t n_partitions = 0) {
        check(shk_shard_preprocess_fastq(h_, comm, file1 ? file1->data() : nullptr, file1 ? file1->size() : 0,
                                         file2 ? file2->data() : nullptr, file2 ? file2->size() : 0, n_partitions, split ? 1 : 0));
    }
    // the same for a rank that staged its packed reads in HBM itself, in several batches of < 2^32 bases each (shk.h:
    // shk_shard_preprocess_batches; no batch: this rank has none)
    struct PackedBatch { const void *d_bases, *d_seg_off; uint64_t n_seg, n_bases; };
    void sharded_preprocess_batches(shk_comm *comm, const std::vector<PackedBatch> &batches, uint64_t n_reads, uint32_t n_partitions = 0) {
        std::vector<const void *> b, s; std::vector<uint64_t> ns, nb;
        for (const PackedBatch &x : batches) { b.push_back(x.d_bases); s.push_back(x.d_seg_off); ns.push_back(x.n_seg); nb.push_back(x.n_bases); }
        check(shk_shard_preprocess_batches(h_, comm, (uint32_t)batches.size(), b.data(), s.data(), ns.data(), nb.data(), n_reads, n_partitions));
    }
    std::string get_preprocessing_info() {
        const char *s = shk_get_preprocessing_info(h_);
        if (!s) throw std::runtime_error(shk_last_error(h_));
        return s;
    }
    void assemble() { check(shk_assemble(h_)); }
    std::string get_assembly() {
        const char *s = shk_get_assembly(h_);
        if (!s) throw std::runtime_error(shk_last_error(h_));
        return s;
    }
    // the outputs as BGZF files, compressed on the device (shk.h: SHK_OUT_FASTA .. SHK_OUT_GFA2; SPEC S11a).  request: before
    // assemble(), the files that will be asked for (bit `which` each); get: the file, whose inflated bytes are the field of
    // get_assembly() with its escapes undone
    void request_assembly_bgzf(uint32_t mask) { check(shk_request_assembly_bgzf(h_, mask)); }
    std::vector<uint8_t> get_assembly_bgzf(int which) {
        const uint8_t *data = nullptr; size_t n = 0;
        check(shk_get_assembly_bgzf(h_, which, &data, &n));
        return std::vector<uint8_t>(data, data + n);
    }
    void on_state(shk_progress_cb cb, void *user) { shk_set_progress_cb(h_, cb, user); }
    shk_handle *raw() { return h_; }

private:
    explicit AssemblyHelper(shk_handle *h) : h_(h) {}
    void check(int rc) { if (rc != SHK_OK) throw std::runtime_error(shk_last_error(h_)); }
    shk_handle *h_;
};

}  // namespace sparrowhawk
