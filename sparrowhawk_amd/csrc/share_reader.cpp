// share_reader.cpp — one rank's share of FASTQ or FASTA files as packed batches in HBM (share_reader.h): read_fastq_share for a
// share of one batch, read_fastq_share_batches for a larger one.  The host's planning (which kind of file, the cuts, the text of
// the share) is share_plan.h's; here are the steps both readers are made of, each written once, and the two readers.
#include "share_reader.h"

#include <algorithm>
#include <utility>

#include "fasta_gpu.h"
#include "handle.h"
#include "inflate_gpu.h"
#include "share_plan.h"

using namespace shk;

namespace {

// ---- route accounting: how a file's slice reached the packer -------------------------------------------------------------
enum Route { None, BgzfSlice, MemberWhole, TextSlice, Host };
const char *const route_name[] = {"", "bgzf_slice", "member_whole", "text_slice", "host"};
void book_route(FastqShare &out, Route r) {
    out.n_bgzf_slice += r == BgzfSlice; out.n_member_whole += r == MemberWhole; out.n_text_slice += r == TextSlice; out.n_host += r == Host;
    if (out.route.find(route_name[r]) == std::string::npos) out.route += (out.route.empty() ? "" : "+") + std::string(route_name[r]);
}

// a text on the device -> one packed batch (0; 1 declined: the host packer owns the messages; < 0)
int device_pack(const ShareFormat &sf, const GpuText &text, uint32_t k, uint32_t min_qual, void *stream, GpuPacked &gp, std::string &err) {
    return sf.fasta() ? gpu_pack_fasta(nullptr, 0, nullptr, 0, k, 0, stream, gp, err, 0, &text) : gpu_pack_fastq(nullptr, 0, nullptr, 0, k, min_qual, 0, stream, gp, err, 0, &text);
}

// ---- slice to device: this file's slice as a span of text in HBM, and which route that was ---------------------------------
// A plain gzip member: inflated whole on the device, then cut.  0: span is the slice; 1: the inflater declined (the host reads
// the file); < 0: the device layer's code.
int member_slice(const SharePlan &pl, const ShareFile &F, int device, void *stream, DevSpan &span, uint64_t &uploaded, std::string &err) {
    Text text;
    if (const int rc = gpu_inflate_member(F.p, F.n, device, stream, text, err)) return rc;
    uploaded += F.n;
    return gpu_text_slice(text, pl.rank, pl.world, stream, span, err, pl.sf.fmt);
}
// Text that is born on the device — a walked chain: the rank's run alone (gpu_bgzf_slice); any other gzip file: member_slice.
// route stays None where the file is not gzip, SHK_GUNZIP_DEVICE=0, or the device declined.  SHK_OK or the error's code.
int device_slice(const SharePlan &pl, int i, const Knobs &kn, int device, void *stream, DevSpan &span, Route &route, uint64_t &uploaded, std::string &err) {
    const ShareFile &F = pl.f[i];
    if (!F.gz || !kn.gunzip_device) return SHK_OK;
    int rc;
    if (F.walked) {
        const char *why = ""; uint64_t up = 0;
        rc = gpu_bgzf_slice(F.p, F.chain, pl.rank, pl.world, device, stream, span, up, why, err, pl.sf.fmt);
        uploaded += up;
    } else rc = member_slice(pl, F, device, stream, span, uploaded, err);
    if (rc < 0) return code_of(Rc::DeviceNoParam, rc);
    if (!rc) route = F.walked ? BgzfSlice : MemberWhole;
    return SHK_OK;
}
// Plain text, or what the device inflater declined: cut on the host, the slice alone is uploaded.
int upload_slice(SharePlan &pl, int i, int device, Text &text, uint64_t &uploaded, std::string &err) {
    if (int rc = pl.host_slice(i, err)) return rc;
    const ShareFile &F = pl.f[i];
    if (int rc = gpu_upload_text(F.t + F.s0, (size_t)(F.s1 - F.s0), device, text, err)) return code_of(Rc::DeviceNoParam, rc);
    uploaded += text.e;
    return SHK_OK;
}

// ---- a packed batch into the share that holds it -----------------------------------------------------------------------
void hold(FastqShare &out, FastqShare::Batch &&b) {
    out.n_seg += b.n_seg; out.n_bases += b.n_bases; out.n_reads += b.n_reads;
    out.batches.push_back(std::move(b));
}
// parsed on the device: b.gp
void hold_device_batch(FastqShare &out, FastqShare::Batch &&b) {
    b.n_seg = b.gp.n_seg; b.n_bases = b.gp.n_bases; b.n_reads = b.gp.n_reads;
    out.n_input_bases += b.gp.n_input_bases;
    hold(out, std::move(b));
}
// parsed on the host: finished and uploaded here.  SHK_OK or SHK_E_OOM (err)
int hold_host_batch(FastqShare &out, PackedReads &pr, std::string &err) {
    FastqShare::Batch b;
    if (upload_packed(pr, b.up, err, &out.uploaded_bytes)) return SHK_E_OOM;
    if (pr.n_seg()) { b.n_seg = pr.n_seg(); b.n_bases = pr.n_bases; }
    b.n_reads = pr.n_reads;
    out.n_input_bases += pr.n_input_bases;
    hold(out, std::move(b));
    return SHK_OK;
}

}  // namespace

// ---- a share of one batch ---------------------------------------------------------------------------------------------------
int read_fastq_share(const uint8_t *fq1, size_t n1, const uint8_t *fq2, size_t n2, uint32_t k, uint32_t min_qual, uint32_t rank,
                     uint32_t world, int device, void *stream, FastqShare &out, std::string &err, bool allow_batches, RecFmt fmt) {
    SharePlan pl;
    if (int rc = plan_share(fmt, fq1, n1, fq2, n2, rank, world, pl, err)) return rc;
    const ShareFormat &sf = pl.sf;
    const Knobs kn;
    const int nf = pl.nf;
    Route route[2] = {None, None};
    // beyond one batch, for the caller that takes batches: nothing is held, read_fastq_share_batches reads the share (again)
    auto in_batches = [&](uint64_t text_ub) -> int {
        err.clear();
        out.batches.clear();
        out.n_seg = out.n_bases = out.n_reads = out.n_input_bases = 0;
        out.in_batches = true; out.text_ub = text_ub;
        return SHK_OK;
    };
    // do this many bases exceed one batch?  Then the caller returns `beyond`: the share goes in batches (its text: text_ub), or SHK_E_PARAM
    int beyond = SHK_OK;
    auto too_large = [&](uint64_t bases, uint64_t text_ub) -> bool {
        if (bases <= kn.batch_bases) return false;
        if (allow_batches) { beyond = in_batches(text_ub); return true; }
        err = std::string(sf.entry()) + ": this rank's share exceeds one batch (SHK_BATCH_BASES = " + std::to_string(kn.batch_bases) +
              " packed bases); several batches per rank are not supported: use more ranks or split the input";
        beyond = SHK_E_PARAM;
        return true;
    };
    if (allow_batches) {
        // decided before anything is uploaded, where the host can tell (estimate_share; a plain member's share is a guess: what it
        // misses is found after the inflation, below)
        if (int rc = estimate_share(pl, err)) return rc;
        if (share_in_batches(sf, pl.total, kn)) return in_batches(pl.total);
    }
    auto finish = [&](bool host_parsed) -> int {
        for (int i = 0; i < nf; i++) book_route(out, host_parsed ? Host : route[i]);
        return SHK_OK;
    };
    if (sf.fasta()) {
        // ---- FASTA: file by file — its slice as a span of text in HBM and the device packer, or the host packer on the host's slice
        // (SHK_HOST_PARSER=1, a host-resident slice below SHK_FASTA_DEVICE_MIN, what the device packer declines)
        uint64_t text_bytes = 0;
        for (int i = 0; i < nf; i++) {
            ShareFile &F = pl.f[i];
            DevSpan span;
            bool on_host = kn.host_parser;
            if (!on_host) if (int rc = device_slice(pl, i, kn, device, stream, span, route[i], out.uploaded_bytes, err)) return rc;
            if (route[i] == None) {
                if (int rc = pl.host_slice(i, err)) return rc;
                route[i] = F.gz ? Host : TextSlice;
                on_host = on_host || F.s1 - F.s0 < kn.fasta_device_min;
                text_bytes += F.s1 - F.s0;
            } else text_bytes += span.len;
            // (a byte is a base: the share goes in batches when its text exceeds one)
            if (too_large(text_bytes, text_bytes)) return beyond;
            FastqShare::Batch b;
            if (!on_host) {
                Text text;
                if (route[i] == BgzfSlice || route[i] == MemberWhole) {
                    if (int rc = gpu_join_spans(&span, 1, stream, text, err)) return code_of(Rc::DeviceNoParam, rc);
                    span.blk.put();
                } else if (int rc = upload_slice(pl, i, device, text, out.uploaded_bytes, err)) return rc;
                const int rc = text.e ? device_pack(sf, text, k, min_qual, stream, b.gp, err) : 0;
                if (rc < 0) return code_of(Rc::Device, rc);
                if (rc) { b.gp.reset(); on_host = true; }    // declined: the host packer owns the message
            }
            if (!on_host) { hold_device_batch(out, std::move(b)); continue; }
            route[i] = Host;
            if (int rc = pl.host_slice(i, err)) return rc;
            PackedReads pr;
            if (int rc = sf.host_pack(F.t + F.s0, (size_t)(F.slice_end() - F.s0), k, min_qual, pr, err)) return code_of(Rc::Parser, rc);
            if (int rc = hold_host_batch(out, pr, err)) return rc;
        }
        if (out.batches.empty()) out.batches.emplace_back();
        return finish(false);
    }
    // ---- FASTQ on the device: every file's slice as a span of text in HBM, joined, parsed
    bool host_parser = kn.host_parser;
    if (!host_parser) {
        DevSpan spans[2];
        for (int i = 0; i < nf; i++) {
            if (int rc = device_slice(pl, i, kn, device, stream, spans[i], route[i], out.uploaded_bytes, err)) return rc;
            if (route[i] != None) continue;
            Text text;
            if (int rc = upload_slice(pl, i, device, text, out.uploaded_bytes, err)) return rc;
            spans[i].len = text.e; spans[i].unterminated = text.unterminated;
            spans[i].blk = PoolBlock(text.d, text.pool_bytes);
            static_cast<GpuText &>(text) = GpuText();      // (the block is the span's now)
            route[i] = pl.f[i].gz ? Host : TextSlice;
        }
        uint64_t bytes = 0;
        for (int i = 0; i < nf; i++) bytes += spans[i].len;
        if (too_large(bytes / 2, bytes)) return beyond;
        Text joined;
        if (int rc = gpu_join_spans(spans, nf, stream, joined, err)) return code_of(Rc::DeviceNoParam, rc);
        for (int i = 0; i < nf; i++) spans[i].blk.put();
        FastqShare::Batch b;
        const int rc = device_pack(sf, joined, k, min_qual, stream, b.gp, err);
        if (rc < 0) return code_of(Rc::Device, rc);
        if (rc == 0) {
            if (too_large(b.gp.n_bases, bytes)) return beyond;
            hold_device_batch(out, std::move(b));
            return finish(false);
        }
        host_parser = true;                               // not regular 4-line FASTQ: the host parser owns the messages
    }
    // ---- the host parser on the same slices
    PackedReads pr;
    for (int i = 0; i < nf; i++) {
        if (int rc = pl.host_slice(i, err)) return rc;
        const ShareFile &F = pl.f[i];
        if (int rc = sf.host_pack(F.t + F.s0, (size_t)(F.slice_end() - F.s0), k, min_qual, pr, err)) return code_of(Rc::Parser, rc);
    }
    uint64_t text = 0;
    for (int i = 0; i < nf; i++) text += pl.f[i].s1 - pl.f[i].s0;
    if (too_large(pr.n_bases, text)) return beyond;
    if (int rc = hold_host_batch(out, pr, err)) return rc;
    return finish(true);
}

// ---- the same share, beyond one batch: batch by batch into pass 1 of the shard layer ------------------------------------------
int read_fastq_share_batches(const uint8_t *fq1, size_t n1, const uint8_t *fq2, size_t n2, uint32_t k, uint32_t min_qual, uint32_t rank,
                             uint32_t world, int device, void *stream, ShardBatchSink &sink, FastqShare &out, std::string &err, RecFmt fmt) {
    SharePlan pl;
    if (int rc = plan_share(fmt, fq1, n1, fq2, n2, rank, world, pl, err)) return rc;
    const ShareFormat &sf = pl.sf;
    const Knobs kn;
    const int nf = pl.nf;
    const uint64_t piece_bytes = sf.piece_bytes(kn);
    if (int rc = estimate_share(pl, err)) return rc;       // (est, total: the progress)
    uint64_t reads = 0, before = 0;                        // the rank's reads so far; the text of the files that are done
    int at_file = 0;
    auto hand = [&](const uint32_t *d_bases, const uint32_t *d_seg_off, uint64_t n_seg, uint64_t n_bases, uint64_t file_done) -> int {
        out.n_batches++; out.n_seg += n_seg; out.n_bases += n_bases;
        const int rc = sink.batch(n_seg ? d_bases : nullptr, n_seg ? d_seg_off : nullptr, n_seg, n_bases, reads, before + std::min(file_done, pl.f[at_file].est), pl.total);
        if (rc) err.clear();
        return rc;
    };
    // a piece of regular text on the device -> parser -> one batch.  DECLINED: not regular 4-line FASTQ (nothing was counted)
    auto device_piece = [&](const GpuText &text, uint64_t file_done) -> int {
        Packed gp;
        const int rc = device_pack(sf, text, k, min_qual, stream, gp, err);
        if (rc < 0) return code_of(Rc::Device, rc);
        if (rc) return DECLINED;
        out.n_windows++;
        reads += gp.n_reads; out.n_reads += gp.n_reads; out.n_input_bases += gp.n_input_bases;
        return hand(gp.d_bases, gp.d_seg_off, gp.n_seg, gp.n_bases, file_done);
    };
    // the host parser from `from` to the end of the slice (its messages count the slice's records: file_reads came before),
    // a batch every SHK_BATCH_BASES bases
    // (FASTA: one piece alone, [from, upto))
    auto host_from = [&](int i, uint64_t from, uint64_t file_reads, uint64_t upto = UINT64_MAX) -> int {
        const ShareFile &F = pl.f[i];
        const uint64_t end = upto < F.s1 ? upto : F.slice_end();
        if (from >= end) return SHK_OK;
        PackedReads pr;
        int flush_rc = SHK_OK;
        uint64_t counted = 0, counted_in = 0;              // reads and input bases of pr that are in the totals already
        auto flush = [&](PackedReads &p, uint64_t file_done) -> int {
            if (p.n_seg() == 0 && p.n_reads == counted) return 0;      // (nothing new)
            reads += p.n_reads - counted; out.n_reads += p.n_reads - counted; counted = p.n_reads;
            out.n_input_bases += p.n_input_bases - counted_in; counted_in = p.n_input_bases;
            UploadedReads up;
            if (upload_packed(p, up, err, &out.uploaded_bytes)) { flush_rc = SHK_E_OOM; return -7; }
            flush_rc = hand((const uint32_t *)up.bases, (const uint32_t *)up.seg_off, p.n_seg(), p.n_bases, file_done);
            p.reset_stream();
            return flush_rc ? -7 : 0;
        };
        const int rc = sf.host_pack(F.t + from, (size_t)(end - from), k, min_qual, pr, err, kn.batch_bases,
                                    [&](PackedReads &p) { return flush(p, from - F.s0); }, file_reads);
        if (rc == -7) return flush_rc;
        if (rc) return code_of(Rc::Parser, rc);
        return flush(pr, std::min(end, F.s1) - F.s0) ? flush_rc : SHK_OK;
    };
    // A span in pieces of at most piece_bytes, each a batch.  span_at: where the span begins in the file's text; file_base: where
    // the slice does (progress).  SHK_OK; DECLINED with `stopped` = the span offset at which the host goes on; an error code.
    auto span_pieces = [&](const DevSpan &span, uint64_t span_at, uint64_t file_base, uint64_t &stopped) -> int {
        for (uint64_t from = 0; from < span.len;) {
            Text piece; uint64_t next = 0;
            const int rc = gpu_span_piece(span, from, piece_bytes, stream, piece, next, err, fmt);
            if (rc < 0) return code_of(Rc::DeviceNoParam, rc);
            if (rc && sf.fasta()) { err = sf.one_record_too_long(next - from, kn); return SHK_E_PARAM; }
            const int prc = rc ? DECLINED : device_piece(piece, span_at + next - file_base);
            if (prc == DECLINED) { stopped = from; return DECLINED; }
            if (prc) return prc;
            from = next;
        }
        return SHK_OK;
    };
    for (int i = 0; i < nf; i++) {
        ShareFile &F = pl.f[i];
        at_file = i;
        Route route = None;
        uint64_t resume = 0;                               // the file's text in front of this offset has been handed over
        bool host_parser = kn.host_parser, through = false;
        const uint64_t reads0 = reads;
        if (!kn.host_parser && F.gz && kn.gunzip_device) {
            if (F.walked) {
                BgzfShareWindows sw;
                const char *why = "";
                int rc = sw.open(F.p, F.chain, rank, world, kn.window.bytes, device, stream, why, err, fmt);
                if (rc < 0) return code_of(Rc::DeviceNoParam, rc);
                while (!rc) {
                    GpuText piece; uint64_t at = 0; bool done = false;
                    rc = sw.next(piece, at, done, why, err);
                    if (rc < 0) return code_of(Rc::DeviceNoParam, rc);
                    if (rc) { resume = sw.consumed(); break; }              // this window is the host reader's, and what follows it
                    route = BgzfSlice;
                    if (done) { through = true; break; }
                    int prc;
                    if (sf.fasta() && piece.e > piece_bytes) {      // a window (and its carry) of more than a batch: in pieces
                        DevSpan view; uint64_t stopped = 0;
                        view.blk = PoolBlock(piece.d, piece.e + 32); view.len = piece.e; view.unterminated = piece.unterminated;
                        prc = span_pieces(view, at, sw.run_begin(), stopped);
                        (void)view.blk.take();                      // (the text stays the windows')
                        if (prc == DECLINED) { resume = at + stopped; host_parser = true; break; }
                    } else {
                        prc = device_piece(piece, at + piece.e - sw.run_begin());
                        if (prc == DECLINED) { resume = at; host_parser = true; break; }
                    }
                    if (prc) return prc;
                }
                out.uploaded_bytes += sw.uploaded();
            } else {
                DevSpan span;
                const int rc = member_slice(pl, F, device, stream, span, out.uploaded_bytes, err);
                if (rc < 0) return code_of(Rc::DeviceNoParam, rc);
                if (!rc) {
                    route = MemberWhole;
                    through = true;
                    uint64_t stopped = 0;
                    const int prc = span_pieces(span, span.off, span.off, stopped);
                    if (prc == DECLINED) { resume = span.off + stopped; host_parser = true; through = false; }
                    else if (prc) return prc;
                }
            }
        }
        if (!through) {
            // plain text, what the device declined, SHK_HOST_PARSER=1: the host's text, cut on the host
            if (int rc = pl.host_slice(i, err)) return rc;
            route = F.gz ? Host : TextSlice;
            uint64_t from = std::max(F.s0, resume);
            // FASTA: the host packer takes pieces too (a record is never split, by either packer), and small slices (SHK_FASTA_DEVICE_MIN)
            const bool host_pieces = sf.fasta() && (host_parser || F.s1 - F.s0 < kn.fasta_device_min);
            while ((!host_parser || host_pieces) && from < F.s1) {
                uint64_t end = F.s1;
                if (F.s1 - from > piece_bytes) {
                    const uint64_t at = sf.last_start(F.t + from, (size_t)piece_bytes);
                    if (sf.fasta() && (at == UINT64_MAX || at == 0)) {
                        const uint64_t nx = fasta_first_record_start(F.t, (size_t)F.s1, (size_t)from + 1);
                        err = sf.one_record_too_long((nx == UINT64_MAX ? F.s1 : nx) - from, kn);
                        return SHK_E_PARAM;
                    }
                    if (at == UINT64_MAX || at == 0) { host_parser = true; break; }      // (no record starts inside the piece)
                    end = from + at;
                }
                if (host_pieces) {
                    route = Host;
                    if (int rc = host_from(i, from, reads - reads0, end)) return rc;
                    from = end;
                    continue;
                }
                Text text;
                if (int rc = gpu_upload_text(F.t + from, (size_t)(end - from), device, text, err)) return code_of(Rc::DeviceNoParam, rc);
                out.uploaded_bytes += text.e;
                const int prc = device_piece(text, end - F.s0);
                if (prc == DECLINED && sf.fasta()) {              // the host packer on this piece: it owns the message
                    route = Host;
                    if (int rc = host_from(i, from, reads - reads0, end)) return rc;
                } else if (prc == DECLINED) { host_parser = true; break; }
                else if (prc) return prc;
                from = end;
            }
            if (host_parser && !sf.fasta()) {
                route = Host;
                if (int rc = host_from(i, from, reads - reads0)) return rc;
            }
        }
        before += F.est;
        book_route(out, route);
    }
    return SHK_OK;
}
