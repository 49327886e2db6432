// share_plan.h — what the host decides about one rank's share of FASTQ or FASTA files before a byte crosses PCIe (the share
// readers, share_reader.cpp): which kind of file each one is, where the rank's nominal cuts lie, how much text the share has
// and whether it goes in batches.  Host code alone — fastq.cpp and zlib behind it, no HIP: tests/cpp/share_plan_main.cpp
// runs it under AddressSanitizer and UBSan.
#pragma once
#include <string>

#include "../../include/shk.h"
#include "read_parts.h"

namespace shk {

// What the record format decides for the share readers: the name in the messages, the slice bounds, the host packer, where
// host pieces are cut, and how many bases a byte of text can hold (FASTQ: half of the text is bases; FASTA: a byte is a base).
struct ShareFormat {
    RecFmt fmt;
    bool fasta() const { return fmt == RecFmt::Fasta; }
    const char *entry() const { return fasta() ? "shard_preprocess_fasta" : "shard_preprocess_fastq"; }
    uint64_t bases_ub(uint64_t text_bytes) const { return fasta() ? text_bytes : text_bytes / 2; }
    uint64_t piece_bytes(const Knobs &kn) const { return fasta() ? kn.batch_bases : 2 * kn.batch_bases; }      // text per piece: its bases fit one batch
    void bounds(const uint8_t *t, size_t e, uint32_t rank, uint32_t world, uint64_t c0, uint64_t c1, uint64_t &s0, uint64_t &s1) const {
        if (fasta()) fasta_slice_bounds(t, e, rank, world, c0, c1, s0, s1); else fastq_slice_bounds(t, e, rank, world, c0, c1, s0, s1);
    }
    uint64_t last_start(const uint8_t *t, size_t n) const { return fasta() ? fasta_last_record_start(t, n) : last_record_start(t, n); }
    int host_pack(const uint8_t *t, size_t n, uint32_t k, uint32_t min_qual, PackedReads &pr, std::string &err, uint64_t flush_bases = 0,
                  const FlushFn &flush = nullptr, uint64_t rec_base = 0) const {
        return fasta() ? pack_fasta(t, n, k, pr, err, 0, nullptr, 0, flush_bases, flush, rec_base) : pack_fastq(t, n, k, min_qual, pr, err, 0, nullptr, 0, flush_bases, flush, rec_base);
    }
    std::string one_record_too_long(uint64_t bytes, const Knobs &kn) const {
        return std::string(entry()) + ": a single FASTA record of " + std::to_string(bytes) + " bytes exceeds one batch (SHK_BATCH_BASES = " +
               std::to_string(kn.batch_bases) + "): a record is never split";
    }
};

// the nominal cuts c_rank and c_(rank + 1) of a walked BGZF chain: the text offsets at which the rank's run and the next begin
inline void bgzf_slice_cuts(const BgzfChain &chain, uint32_t rank, uint32_t world, uint64_t &c0, uint64_t &c1) {
    std::vector<uint32_t> isize(chain.blocks.size());
    for (size_t i = 0; i < isize.size(); i++) isize[i] = chain.blocks[i].isize;
    std::vector<uint64_t> first;
    plan_fastq_slices(isize.data(), isize.size(), world, first);
    uint64_t off = 0;
    c0 = c1 = chain.text;
    for (size_t b = 0; b <= isize.size(); b++) {
        if (b == first[rank]) c0 = off;
        if (b == first[rank + 1]) { c1 = off; break; }
        if (b < isize.size()) off += isize[b];
    }
}

// One file of the share as the host sees it.
struct ShareFile {
    const uint8_t *p = nullptr; size_t n = 0;             // the file as it was given
    bool gz = false, walked = false;                       // gzip magic; walked: a complete BGZF chain — its cuts lie at block starts, on every route
    BgzfChain chain;
    uint64_t c0 = 0, c1 = 0;                               // the nominal cuts of (rank, world): known at once for a walked chain, else with the host's text
    ByteVec st; const uint8_t *t = nullptr; size_t l = 0, e = 0; bool host_text = false;      // the host's text, read once; e: without its trailing blank lines
    uint64_t s0 = 0, s1 = 0;                               // the slice inside the host text
    uint64_t est = 0;                                      // bytes of text of the slice, as far as known beforehand (estimate_share)
    // The end of the slice for the host packers.  A slice that reaches the end of the text takes the blank lines behind it
    // along: trimmed_len cannot tell a blank line from the line end that closes the empty quality line of a last record
    // without bases, and the parser skips the others.
    uint64_t slice_end() const { return s1 == e ? l : s1; }
};
struct SharePlan {
    ShareFormat sf{RecFmt::Fastq};
    uint32_t rank = 0, world = 1;
    int nf = 0;
    ShareFile f[2];
    uint64_t total = 0;                                    // the sum of the files' est
    // the host's text of file i (read once) and the slice in it.  SHK_OK, or the code of a damaged stream (err)
    int host_slice(int i, std::string &err) {
        ShareFile &F = f[i];
        if (F.host_text) return SHK_OK;
        if (int ri = maybe_inflate(F.p, F.n, F.st, F.t, F.l, err)) return ri == -3 ? SHK_E_PARSE : SHK_E_OOM;
        F.e = trimmed_len(F.t, F.l);
        if (!F.walked) { F.c0 = slice_cut(F.e, rank, world); F.c1 = slice_cut(F.e, rank + 1, world); }
        sf.bounds(F.t, F.e, rank, world, F.c0, F.c1, F.s0, F.s1);
        F.host_text = true;
        return SHK_OK;
    }
};

// The one or two files of a share: the argument checks of both readers (SHK_E_PARAM with its message in err), then what each
// file is.  Nothing is inflated here.
inline int plan_share(RecFmt fmt, const uint8_t *fq1, size_t n1, const uint8_t *fq2, size_t n2, uint32_t rank, uint32_t world, SharePlan &out, std::string &err) {
    out.sf = ShareFormat{fmt};
    if ((!fq1 && (n1 || fq2)) || (!fq2 && n2)) { err = std::string(out.sf.entry()) + ": a null file with a size, or a second file without a first"; return SHK_E_PARAM; }
    if (world == 0 || rank >= world) { err = std::string(out.sf.entry()) + ": rank beyond world"; return SHK_E_PARAM; }
    out.rank = rank; out.world = world;
    out.nf = fq2 ? 2 : (fq1 ? 1 : 0);
    out.f[0].p = fq1; out.f[0].n = n1; out.f[1].p = fq2; out.f[1].n = fq2 ? n2 : 0;
    for (int i = 0; i < out.nf; i++) {
        ShareFile &F = out.f[i];
        F.gz = F.n >= 18 && F.p[0] == 0x1F && F.p[1] == 0x8B;
        size_t bs = 0; const char *why = "";
        F.walked = F.gz && bgzf_block(F.p, F.n, bs) && bgzf_walk(F.p, F.n, F.chain, why) == 0;
        if (F.walked) bgzf_slice_cuts(F.chain, rank, world, F.c0, F.c1);
    }
    return SHK_OK;
}

// How much text the share has, as far as the host can tell before anything is uploaded: the ISIZE sum of the rank's run of a
// walked chain, a plain member's ISIZE field over the ranks (a guess), the slice bounds of plain text (which is read for it).
inline int estimate_share(SharePlan &pl, std::string &err) {
    pl.total = 0;
    for (int i = 0; i < pl.nf; i++) {
        ShareFile &F = pl.f[i];
        if (F.walked) F.est = F.c1 - F.c0;
        else if (F.gz) { const uint8_t *t = F.p + F.n - 4; F.est = (t[0] | ((uint64_t)t[1] << 8) | ((uint64_t)t[2] << 16) | ((uint64_t)t[3] << 24)) / pl.world; }
        else { if (int rc = pl.host_slice(i, err)) return rc; F.est = F.s1 - F.s0; }
        pl.total += F.est;
    }
    return SHK_OK;
}

// does a share of this much text go in batches (a share whose bases may exceed one batch does)
inline bool share_in_batches(const ShareFormat &sf, uint64_t text, const Knobs &kn) { return sf.bases_ub(text) > kn.batch_bases; }

}  // namespace shk
