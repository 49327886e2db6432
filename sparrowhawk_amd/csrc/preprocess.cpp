// preprocess.cpp — how reads reach the counting passes.  shk_preprocess tries these routes in this order; a route fails
// (error set, SHK_E_*), handles the input, or declines having counted nothing, and the next one is tried:
//     (plan_device_gunzip, where every file starts with the gzip magic, SHK_GUNZIP_DEVICE != 0 and SHK_HOST_PARSER != 1,
//      picks ONE of the first two before anything is uploaded; its decline goes on to route 3)
//   1 route_device_gzip          device inflater (a plain member or a BGZF file) -> device parser -> one batch.  Declines when the
//                                inflater or the parser declines or the text exceeds one batch.
//   2 route_device_bgzf_windows  every file is a BGZF chain from its first byte to its last whose text (the sum of the blocks'
//                                ISIZE fields) is more than route 1 takes: beyond one batch, a file of 4 GiB or more, or beyond
//                                SHK_GUNZIP_DEVICE_WINDOW where that is set.  Window by window (inflate_gpu.h: BgzfWindows —
//                                upload, inflate, cut at the last record start), parse, one batch each.  The size is looked at
//                                FIRST, so such a file never enters route 1; a decline (window 0 damaged or not regular) goes
//                                on below.
//     (what is gzip is inflated on the host here, once, for the routes below)
//   3 route_device_pieces(one)   the text fits one batch and is >= SHK_FASTQ_PIPELINE_MIN (64 MiB): cut into a few pieces,
//                                piece i+1 uploaded while piece i is parsed, counted as ONE batch
//   4 route_device_single        the text fits one batch (and route 3 has not found it irregular): one upload, one parse
//   5 route_device_pieces        the text exceeds one batch: one batch per piece
//   6 route_host                 SHK_HOST_PARSER=1, or every route above declined.  Never declines.
//   7 push_reads_impl            the streaming entry point: the device parser for a chunk of >= SHK_STREAM_DEVICE_MIN bytes
//                                that is regular 4-line FASTQ, else the host parser
//   8 read_fastq_share           } the sharded entry points from files (shk_shard_preprocess_fastq / _fasta): one rank's slice of every
//   9 read_fastq_share_batches   } file as one packed batch, or batch by batch — share_reader.cpp (share_reader.h says how)
// The device parser (fastq_gpu.hip) takes regular 4-line FASTQ only; irregular framing and every malformed record go to
// the host parser (fastq.cpp), which owns the error messages.
#include "preprocess.h"

#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <thread>
#include <utility>
#include <vector>

#include "fasta_gpu.h"
#include "fastq_gpu.h"
#include "inflate_gpu.h"
#include "inflate_mt.h"
#include "read_parts.h"

namespace shk { bool spectrum_fit(const uint64_t *histo500, uint32_t *out); }   // fit.cpp

using namespace shk;

uint32_t emit_threshold_of(const shk_handle *h) {
    // the fit never returns less than 1 and falls back to min_count (SPEC S6)
    return h->do_fit ? (h->min_count < 1u ? h->min_count : 1u) : h->min_count;
}

namespace {

// where a text lies in the whole input: the percentage of a `loop:<n>:<pct>` string (the streaming entry point posts none)
struct Span { uint64_t base = 0, total = 0; bool pct = true; };
void post_loop(shk_handle *h, uint64_t reads, const Span &sp, uint64_t bytes) {
    std::string s = "loop:" + std::to_string(reads);
    if (sp.pct) s += ":" + std::to_string(sp.total ? (100 * (sp.base + bytes)) / sp.total : 100);
    h->post_mode(s.c_str());
}
// the marks of a device-parsed batch: one every `every` reads, with the bytes consumed inside the file the mark lies in
// (bit 63: the second file of a single-shot pair, which starts n1 bytes into the input)
void post_device_progress(shk_handle *h, const GpuPacked &gp, const Span &sp, uint64_t n1 = 0) {
    const uint64_t every = h->progress_every();
    for (size_t j = 0; j < gp.progress_bytes.size(); j++) {
        const bool second = (gp.progress_bytes[j] >> 63) != 0;
        post_loop(h, every * (gp.first_mark + j + 1), sp, (second ? n1 : 0) + (gp.progress_bytes[j] & ~(1ull << 63)));
    }
}

// one batch of packed segments in HBM -> pass 1 (several batches per handle are allowed)
int count_one_batch(shk_handle *h, const uint32_t *d_bases, const uint32_t *d_seg_off, uint64_t n_seg, uint64_t n_bases) {
    std::string err;
    const double t0 = now_ms();
    h->batches_started++;
    int rc = h->pipe->count_batch(d_bases, d_seg_off, n_seg, n_bases, err);
    // (not through times(): that waits for the event behind pass 1 when pass 1 was not waited for, and pass 2, which
    // finish_counting is about to launch behind it, would reach the GPU late)
    h->pipe->add_time("preprocess_device_total_host_clock", now_ms() - t0);
    return rc ? fail_rc(h, Rc::Device, rc, err) : SHK_OK;
}
// the packed pieces of ONE batch -> pass 1 (the pieces with no segment are left out by the caller)
int count_pieces(shk_handle *h, const std::vector<DevPiece> &pcs) {
    std::string err;
    const double t0 = now_ms();
    h->batches_started++;
    const int rc = h->pipe->count_batch_pieces(pcs.data(), pcs.size(), err);
    h->pipe->add_time("preprocess_device_total_host_clock", now_ms() - t0);
    return rc ? fail_rc(h, Rc::Device, rc, err) : SHK_OK;
}

// common tail of every preprocess entry point: all batches are in -> histogram, fit, filter
int finish_counting(shk_handle *h) {
    std::string err;
    const double t0 = now_ms();
    h->post_loop_edge("loop:end");
    if (!h->do_bloom && h->chunk_size == 0) h->post("preprocess:bulk:sorting");
    int rc = h->pipe->histogram(h->histo, emit_threshold_of(h), err);
    if (rc) return fail(h, SHK_E_DEVICE, err);
    h->used_min_count = h->min_count; h->fit_ok = false;
    if (h->do_fit) {
        h->post_mode("fitting");
        uint32_t v = 0;
        if (spectrum_fit(h->histo, &v)) { h->used_min_count = v; h->fit_ok = true; }
    }
    h->post_mode("filtering");
    rc = h->pipe->filter(h->used_min_count, err);
    if (rc) return fail_rc(h, Rc::DeviceNoParam, rc, err);
    h->post("preprocess:saving");
    h->pre_json = preprocessing_json(h->pipe->n_solid(), h->histo, h->used_min_count);
    h->pipe->times().add("preprocess_device_total_host_clock", now_ms() - t0);
    h->st = St::Preprocessed;
    h->post("preprocess:end");
    return SHK_OK;
}

// one batch, and the caller's reads stay in place until this function returns: the two counting passes run back to back
int run_counting(shk_handle *h, const uint32_t *d_bases, const uint32_t *d_seg_off, uint64_t n_seg, uint64_t n_bases) {
    h->pipe->single_batch_resident(true);
    int rc = count_one_batch(h, d_bases, d_seg_off, n_seg, n_bases);
    if (!rc) rc = finish_counting(h);
    h->pipe->single_batch_resident(false);
    return rc;
}

// hand the packed stream on as one batch (upload + pass 1) and empty it; read counters are kept
int flush_host_batch(shk_handle *h, PackedReads &pr) {
    if (pr.n_seg() == 0) { pr.reset_stream(); return SHK_OK; }
    std::string err;
    UploadedReads up;
    pr.finish();                                          // (in front of the clock, which times the upload alone)
    const double t0 = now_ms();
    if (upload_packed(pr, up, err)) return fail(h, SHK_E_OOM, err);
    h->pipe->times().add("h2d_upload_host_clock", now_ms() - t0);
    const int rc = count_one_batch(h, (const uint32_t *)up.bases, (const uint32_t *)up.seg_off, pr.n_seg(), pr.n_bases);
    pr.reset_stream();
    return rc;
}

// chunked mode hands a batch on every chunk_size reads (docs/src/assembly.md:17: "reads per batch")
uint64_t flush_every_reads(const shk_handle *h) { return (!h->do_bloom && h->chunk_size > 0) ? h->chunk_size : 0; }

// The host parser over one text, appended to `pr`: progress is posted as it goes, and a batch is handed on every
// flush_reads reads (0 = never) or batch_bases bases.  What is left in `pr` at the end is the caller's to flush.
// rec_base: records of this file that came before the text (numbering of the error messages).
int host_parse(shk_handle *h, const Knobs &kn, const uint8_t *t, size_t n, PackedReads &pr, const Span &sp, uint64_t flush_reads, uint64_t rec_base = 0) {
    std::string err;
    auto prog = [&](uint64_t reads, uint64_t bytes, uint64_t) { post_loop(h, reads, sp, bytes); };
    int flush_rc = SHK_OK;
    auto flush = [&](PackedReads &p) -> int { flush_rc = flush_host_batch(h, p); return flush_rc ? -7 : 0; };
    const int rc = pack_fastq(t, n, h->k, h->min_qual, pr, err, h->progress_every(), prog, flush_reads, kn.batch_bases, flush, rec_base);
    if (rc == -7) return flush_rc;                       // the batch hand-over failed: its error is set
    return rc ? fail_rc(h, Rc::Parser, rc, err) : SHK_OK;
}

// The rest of a file through the host parser, as a batch of its own: t[0..n) with the record numbers of the whole file
// (file_reads came before it); reads_done goes in and comes out.
int host_rest(shk_handle *h, const Knobs &kn, const uint8_t *t, size_t n, const Span &sp, uint64_t file_reads, uint64_t &reads_done) {
    PackedReads pr;
    pr.n_reads = reads_done;
    if (int rc = host_parse(h, kn, t, n, pr, sp, 0, file_reads)) return rc;
    if (int rc = flush_host_batch(h, pr)) return rc;
    reads_done = pr.n_reads;
    return SHK_OK;
}

// the device parser on a text that lies on the device already (0, 1 not regular 4-line FASTQ, < 0: as gpu_pack_fastq)
int parse_device_text(shk_handle *h, const GpuText &text, uint64_t reads_done, GpuPacked &gp, std::string &err) {
    return gpu_pack_fastq(nullptr, 0, nullptr, 0, h->k, h->min_qual, h->progress_every(), h->pipe->stream(), gp, err, reads_done, &text);
}
// a device-parsed batch is in: its progress marks, its reads, pass 1 (nothing to count without a segment), its blocks go back
int device_batch_in(shk_handle *h, Packed &gp, const Span &sp, uint64_t &reads_done, uint64_t *file_reads = nullptr /* of the file the batch lies in */) {
    post_device_progress(h, gp, sp);
    reads_done += gp.n_reads;
    if (file_reads) *file_reads += gp.n_reads;
    const int rc = gp.n_seg ? count_one_batch(h, gp.d_bases, gp.d_seg_off, gp.n_seg, gp.n_bases) : SHK_OK;
    gp.reset();
    return rc;
}

// start of the first FASTQ record at or after `from` (a line starting with '@' whose line after next starts
// with '+': a quality line may start with '@' too, but then the line after next is a sequence); n = none,
// SIZE_MAX = the text does not look like 4-line FASTQ here
size_t next_record_start(const uint8_t *t, size_t n, size_t from) {
    size_t p = from;
    if (p >= n) return n;
    if (p > 0 && t[p - 1] != '\n') {
        const void *nl = memchr(t + p, '\n', n - p);
        if (!nl) return n;
        p = (size_t)((const uint8_t *)nl - t) + 1;
    }
    for (int tries = 0; tries < 8 && p < n; tries++) {
        const void *e0 = memchr(t + p, '\n', n - p);
        if (!e0) return n;
        const size_t b = (size_t)((const uint8_t *)e0 - t) + 1;
        if (b >= n) return n;
        const void *e1 = memchr(t + b, '\n', n - b);
        if (!e1) return n;
        const size_t c = (size_t)((const uint8_t *)e1 - t) + 1;
        if (t[p] == '@' && c < n && t[c] == '+') return p;
        p = b;
    }
    return SIZE_MAX;
}

// what shk_preprocess was given, (routes 1 and 2) its BGZF chains as plan_device_gunzip walked them, and (from route 3 on) its text
struct Input {
    const uint8_t *fq1, *fq2; size_t n1, n2, total;     // fq2 null: one file; total: the bytes given, the denominator of the progress percentages
    double t0;                                           // when the entry point started
    ByteVec st1, st2;
    const uint8_t *t1 = nullptr, *t2 = nullptr; size_t l1 = 0, l2 = 0;      // the plain text (t2 null, l2 0: one file)
    size_t text_total() const { return l1 + l2; }
    BgzfChain chain[2]; bool walked[2] = {false, false};      // a file that is a complete BGZF chain: the inflaters do not walk it again
};

// Before routes 1 and 2, and before anything is uploaded: 0 some file lacks the gzip magic (neither route), 2 every file is
// a complete BGZF chain (fastq.h: bgzf_walk; the chains stay in `in`) whose text — the sum of the blocks' ISIZE
// fields — is more than route 1 takes and can be cut into windows, 1 otherwise.
int plan_device_gunzip(const Knobs &kn, Input &in) {
    const uint8_t *gz[2] = {in.fq1, in.fq2}; const size_t gn[2] = {in.n1, in.fq2 ? in.n2 : 0};
    const int nf = in.fq2 ? 2 : 1;
    for (int f = 0; f < nf; f++) if (gn[f] < 18 || gz[f][0] != 0x1F || gz[f][1] != 0x8B) return 0;
    uint64_t total = 0; bool chains = true, wants = false;
    for (int f = 0; f < nf; f++) {
        const char *why = "";
        size_t bs = 0;
        in.walked[f] = bgzf_block(gz[f], gn[f], bs) && bgzf_walk(gz[f], gn[f], in.chain[f], why) == 0;
        chains = chains && in.walked[f];
        total += in.chain[f].text;
        wants = wants || in.chain[f].text >= (1ull << 32) || (kn.window.set && in.chain[f].text > kn.window.bytes);
    }
    if (!chains || total == 0 || !(wants || total / 2 > kn.batch_bases)) return 1;
    for (int f = 0; f < nf; f++) if (bgzf_cut_windows(in.chain[f], kn.window.bytes)) return 1;
    return 2;
}

// Route 1.  Both files (or the one) are what the device inflater takes — a plain gzip member or a BGZF chain, in any
// combination within a pair.  Declines (nothing counted) when any file is not taken or turns out not to be regular
// 4-line FASTQ: the host reader then starts over.  (The progress of file 1 is posted before file 2 is parsed, so a
// decline over file 2 leaves marks behind that the later route posts again.)
int route_device_gzip(shk_handle *h, const Knobs &kn, const Input &in) {
    const uint8_t *gz[2] = {in.fq1, in.fq2}; const size_t gn[2] = {in.n1, in.fq2 ? in.n2 : 0};
    const int nf = in.fq2 ? 2 : 1;
    std::string err;
    const double t0 = now_ms();
    Text text[2]; Packed packed[2];
    double ms_h2d = 0, ms_search = 0, ms_decode = 0, ms_resolve = 0;
    uint64_t bgzf_blocks = 0;
    for (int f = 0; f < nf; f++) {
        GpuInflateStats st;
        const int rc = gpu_inflate_member(gz[f], gn[f], h->pipe->device(), h->pipe->stream(), text[f], err, &st, false, in.walked[f] ? &in.chain[f] : nullptr);
        if (rc == 1) { h->pipe->times().add("gunzip_device_not_taken_x1", 1.0); return DECLINED; }
        if (rc) return fail_rc(h, Rc::DeviceNoParam, rc, err);
        ms_h2d += st.h2d_ms; ms_search += st.search_ms; ms_decode += st.decode_ms; ms_resolve += st.resolve_ms;
        bgzf_blocks += st.blocks;
    }
    const double t1 = now_ms();
    Span sp;                                             // progress as the text path posts it, with the share of the (inflated) text consumed so far
    for (int f = 0; f < nf; f++) sp.total += text[f].e;
    if (sp.total / 2 > kn.batch_bases) return DECLINED;  // (several batches: the host reader's piece-wise path)
    uint64_t reads_done = 0;
    for (int f = 0; f < nf; f++) {
        const int rc = parse_device_text(h, text[f], reads_done, packed[f], err);
        if (rc < 0) return fail_rc(h, Rc::Device, rc, err);
        if (rc == 1) { h->pipe->times().add("gunzip_device_not_taken_x1", 1.0); return DECLINED; }      // not regular FASTQ: the host parser owns the messages
        post_device_progress(h, packed[f], sp);
        reads_done += packed[f].n_reads;
        sp.base += text[f].e;
        h->pipe->times().add("fastq_device_kernels", packed[f].kernels_ms);
        text[f].reset();
    }
    h->pipe->times().add("gunzip_device_host_clock", t1 - t0);
    h->pipe->times().add("gunzip_device_h2d", ms_h2d);
    h->pipe->times().add("gunzip_device_search", ms_search);
    h->pipe->times().add("gunzip_device_decode", ms_decode);
    h->pipe->times().add("gunzip_device_windows_resolve_crc", ms_resolve);
    h->pipe->times().add("gunzip_device_members_x1", (double)nf);
    if (bgzf_blocks) h->pipe->times().add("gunzip_device_bgzf_blocks_x1", (double)bgzf_blocks);      // non-empty BGZF blocks, one wave each
    h->pipe->times().add("fastq_device_parse_pack_host_clock", now_ms() - t1);
    h->n_reads = reads_done;
    std::vector<DevPiece> pcs;
    for (int f = 0; f < nf; f++) if (packed[f].n_seg) pcs.push_back(DevPiece{packed[f].d_bases, packed[f].d_seg_off, packed[f].n_seg, packed[f].n_bases});
    const int rc = count_pieces(h, pcs);
    return rc ? rc : finish_counting(h);
}

// Route 2.  Every file is a complete BGZF chain whose text is more than route 1 takes (plan_device_gunzip).  A window is a
// run of consecutive blocks of at most kn.window bytes of text: BgzfWindows::step uploads its compressed bytes while the
// window before it is worked on, inflates it behind the carry (the partial record the window before it ended in) and cuts
// it at its last record start on the device; here it is parsed and counted as a batch of its own.
// Declines while nothing is counted: window 0 damaged or not regular 4-line FASTQ, no device memory.  Later, whatever goes
// wrong with a window sends the rest of its file, from that window's first block on and with the carry in front, through
// the host reader and the host parser, which own the messages (host_rest); a carry never crosses from file 1 to file 2.
int route_device_bgzf_windows(shk_handle *h, const Knobs &kn, const Input &in) {
    const uint8_t *gz[2] = {in.fq1, in.fq2}; const size_t gn[2] = {in.n1, in.fq2 ? in.n2 : 0};
    const int nf = in.fq2 ? 2 : 1;
    const BgzfChain (&chain)[2] = in.chain;
    const uint64_t total = chain[0].text + (nf == 2 ? chain[1].text : 0);
    std::string err;
    struct Book {                                         // the timings, on every way out
        shk_handle *h; double h2d = 0, decode = 0, kernels = 0; uint64_t windows = 0, blocks = 0; int nf = 1;
        ~Book() {
            if (!windows) return;
            auto &t = h->pipe->times();
            t.add("gunzip_device_windows_x1", (double)windows); t.add("gunzip_device_bgzf_blocks_x1", (double)blocks);
            t.add("gunzip_device_members_x1", (double)nf);
            t.add("gunzip_device_h2d", h2d); t.add("gunzip_device_decode", decode); t.add("fastq_device_kernels", kernels);
        }
    } book{h}; book.nf = nf;
    uint64_t reads_done = 0, text_before_file = 0;
    bool counted_any = false;
    for (int f = 0; f < nf; f++) {
        const std::vector<BgzfChain::Window> &wins = chain[f].windows;
        uint64_t file_reads = 0, carry = 0;
        std::vector<uint8_t> carry_host;                  // the carry in front of the current window, for the host reader
        BgzfWindows bw;
        // (this file's share of the two sums, on every way out of the file)
        struct Sum { Book &b; BgzfWindows &w; ~Sum() { b.h2d += w.h2d_ms; b.decode += w.decode_ms; } } sum{book, bw};
        // what the device does not do with window w: nothing is counted yet -> decline; else the host reader takes the file
        // from that window's first block on, the carry in front
        auto give_up = [&](size_t w) -> int {
            bw.close();
            if (!counted_any) return DECLINED;
            const BgzfChain::Window &win = wins[w];
            ByteVec st; const uint8_t *p = nullptr; size_t pn = 0;
            const double th = now_ms();
            if (int ri = maybe_inflate(gz[f] + win.in_off, gn[f] - (size_t)win.in_off, st, p, pn, err)) return fail_rc(h, Rc::Inflater, ri, err);
            h->pipe->times().add("gunzip_host_clock", now_ms() - th);
            ByteVec joined;
            if (!carry_host.empty()) {
                joined.resize(carry_host.size() + pn);
                memcpy(joined.data(), carry_host.data(), carry_host.size()); memcpy(joined.data() + carry_host.size(), p, pn);
                p = joined.data(); pn = joined.size();
            }
            return host_rest(h, kn, p, pn, Span{text_before_file + win.text_before - carry_host.size(), total}, file_reads, reads_done);
        };
        int rc = bw.open(gz[f], &chain[f], h->pipe->device(), h->pipe->stream(), err);
        if (rc < 0) return fail_rc(h, Rc::DeviceNoParam, rc, err);
        bool to_host = rc == 1;
        size_t w = 0;
        for (; !to_host && w < wins.size(); w++) {
            const Span sp{text_before_file + wins[w].text_before - carry, total};
            const char *why = "";                         // (for a debugger: the host reader words the message)
            GpuText text;                                 // (the buffer stays bw's)
            uint64_t cut = 0;
            rc = bw.step(w, false, carry, cut, text.unterminated, why, err);
            if (rc < 0) return fail_rc(h, Rc::DeviceNoParam, rc, err);
            if ((to_host = rc == 1)) break;
            Packed gp;
            if (cut) {
                text.d = bw.text(w); text.e = (size_t)cut;
                rc = parse_device_text(h, text, reads_done, gp, err);
                if (rc < 0) return fail_rc(h, Rc::Device, rc, err);
                if ((to_host = rc == 1)) break;           // not regular FASTQ: the host parser owns the messages
            }
            book.windows++; book.blocks += wins[w].nonempty;
            if (cut) {
                if (!counted_any) h->pipe->expect_more_batches();
                counted_any = true;
                book.kernels += gp.kernels_ms;
                if (int rc2 = device_batch_in(h, gp, sp, reads_done, &file_reads)) return rc2;
            }
            // the carry as the host would need it
            carry_host.resize((size_t)carry);
            if (carry && device_download(carry_host.data(), bw.text(w + 1), (size_t)carry, err)) return fail(h, SHK_E_DEVICE, err);
        }
        if (to_host) if (int r = give_up(w)) return r;  // (0: the rest of this file is done)
        text_before_file += chain[f].text;
    }
    h->n_reads = reads_done;
    return finish_counting(h);
}

// Routes 3 and 5.  The text is cut at record boundaries into pieces that go through the device parser one after the
// other; a helper thread uploads piece i+1 while piece i is parsed and counted (H2D is two thirds of the entry point).
// Route 5 (a text of more than one batch): pieces of ~2 * batch_bases bytes, each counted as its own batch (pass 1)
// before the next is parsed.  Route 3 (one_batch: the text fits one batch): SHK_FASTQ_PIECES pieces, kept and counted
// together as ONE batch at the end (pass 1 runs over the pieces into the same slices: the partitioning of a single
// batch, no batch packing, no merge).
// Declines (nothing counted) when the very first piece is not regular 4-line FASTQ.  A later piece that is not
// regular is parsed on the host from there to the end of its file, with the record numbers and progress of the
// whole file.
int route_device_pieces(shk_handle *h, const Knobs &kn, const Input &in, bool one_batch) {
    std::string err;
    const uint8_t *const text[2] = {in.t1, in.t2}; const size_t len[2] = {in.l1, in.l2};
    size_t piece_bytes = (size_t)(2 * kn.batch_bases);
    if (one_batch) {
        // the last piece is parsed with nothing left to upload: it is the small one (a tenth of the text)
        const size_t C = kn.pieces, tot = in.text_total();
        piece_bytes = std::max<size_t>(C >= 3 ? tot / 10 * 9 / (C - 1) : tot / C, 1024);
    }
    struct Piece { int file; size_t off, end; bool host_rest; };
    std::vector<Piece> pieces;
    for (int f = 0; f < 2; f++)
        for (size_t off = 0, end; text[f] && off < len[f]; off = end) {
            end = len[f];
            if (len[f] - off > piece_bytes + piece_bytes / 8) {
                end = next_record_start(text[f], len[f], off + piece_bytes);
                if (end == SIZE_MAX || end <= off) { pieces.push_back(Piece{f, off, len[f], true}); break; }   // no record boundary: host from here
            }
            pieces.push_back(Piece{f, off, end, false});
        }
    std::vector<Packed> kept;                             // one_batch: the parsed pieces, counted together
    auto count_kept = [&]() -> int {
        if (kept.empty()) return SHK_OK;
        std::vector<DevPiece> pcs;
        for (auto &g : kept) pcs.push_back(DevPiece{g.d_bases, g.d_seg_off, g.n_seg, g.n_bases});
        const int rc = count_pieces(h, pcs);
        kept.clear();
        return rc;
    };
    const int device = h->pipe->device();
    uint64_t reads_done = 0, file_reads = 0;
    bool counted_any = false;
    const double t0 = now_ms();
    Text cur, nxt;
    // (declared after the texts: joined before they are released, on every way out, exceptions included)
    struct Uploader { int rc = 0; std::string err; std::thread t; void join() { if (t.joinable()) t.join(); } ~Uploader() { join(); } } upl;
    // the rest of a file through the host parser (a piece that is not regular 4-line FASTQ, or no boundary found)
    auto rest_on_host = [&](const Piece &pc) -> int {
        if (int rc = count_kept()) return rc;             // (one_batch: what the device parsed so far is a batch of its own now)
        if (!counted_any) h->pipe->expect_more_batches();
        counted_any = true;
        return host_rest(h, kn, text[pc.file] + pc.off, len[pc.file] - pc.off, Span{(pc.file ? in.n1 : 0) + pc.off, in.total}, file_reads, reads_done);
    };
    for (size_t i = 0; i < pieces.size(); i++) {
        const Piece pc = pieces[i];
        if (i == 0 || pieces[i - 1].file != pc.file) file_reads = 0;
        if (pc.host_rest) {
            if (!counted_any && i == 0) return DECLINED;
            if (int rc = rest_on_host(pc)) return rc;
            continue;
        }
        if (!cur.d)
            if (int rc = gpu_upload_text(text[pc.file] + pc.off, pc.end - pc.off, device, cur, err)) return fail_rc(h, Rc::DeviceNoParam, rc, err);
        // the next piece travels while this one is parsed and counted
        const bool prefetch = i + 1 < pieces.size() && !pieces[i + 1].host_rest;
        if (prefetch)
            upl.t = std::thread([&, nx = pieces[i + 1]]() {
                MemGuard mg(h->mem);                       // (the text block this thread allocates belongs to the handle)
                try { upl.rc = gpu_upload_text(text[nx.file] + nx.off, nx.end - nx.off, device, nxt, upl.err); }
                catch (...) { upl.rc = -4; upl.err = "out of host memory (uploader)"; }
            });
        Packed gp;
        const double tp0 = now_ms();
        int rc = parse_device_text(h, cur, reads_done, gp, err);
        h->pipe->times().add("fastq_piece_parse_host_clock", now_ms() - tp0);
        if (rc < 0) return fail_rc(h, Rc::Device, rc, err);
        if (rc == 1) {
            gp.reset();
            upl.join(); cur.reset(); nxt.reset();
            if (!counted_any) return DECLINED;
            if (int rc2 = rest_on_host(Piece{pc.file, pc.off, len[pc.file], true})) return rc2;
            while (i + 1 < pieces.size() && pieces[i + 1].file == pc.file) i++;      // the rest of this file is done
            continue;
        }
        if (!counted_any && !one_batch) h->pipe->expect_more_batches();
        h->pipe->times().add("fastq_h2d_text", gp.h2d_ms);
        h->pipe->times().add("fastq_device_kernels", gp.kernels_ms);
        h->pipe->times().add("fastq_device_pieces_x1", 1.0);
        const Span sp{(pc.file ? in.n1 : 0) + pc.off, in.total};
        if (one_batch) {                                  // (counted with the other pieces at the end)
            post_device_progress(h, gp, sp);
            reads_done += gp.n_reads; file_reads += gp.n_reads;
            kept.push_back(std::move(gp));
        } else if (int rc2 = device_batch_in(h, gp, sp, reads_done, &file_reads)) return rc2;
        counted_any = true;
        // hand over to the uploaded next piece
        const double tj0 = now_ms();
        upl.join();
        h->pipe->times().add("fastq_piece_wait_for_upload_host_clock", now_ms() - tj0);
        cur.reset();
        if (prefetch && upl.rc) return fail_rc(h, Rc::DeviceNoParam, upl.rc, upl.err);
        if (prefetch) cur = std::move(nxt);
    }
    h->pipe->times().add("fastq_device_parse_pack_host_clock", now_ms() - t0);
    if (int rc = count_kept()) return rc;
    h->n_reads = reads_done;
    return finish_counting(h);
}

// Route 4.  The whole text (both files) in one upload and one parse.  Declines when it is not regular 4-line FASTQ.
int route_device_single(shk_handle *h, const Knobs &, const Input &in) {
    std::string err;
    const double t0 = now_ms();
    Packed gp;
    const int rc = gpu_pack_fastq(in.t1, in.l1, in.t2, in.l2, h->k, h->min_qual, h->progress_every(), h->pipe->stream(), gp, err);
    if (rc < 0) return fail_rc(h, Rc::Device, rc, err);
    if (rc == 1) return DECLINED;
    h->pipe->times().add("fastq_device_parse_pack_host_clock", now_ms() - t0);
    h->pipe->times().add("fastq_h2d_text", gp.h2d_ms);
    h->pipe->times().add("fastq_device_kernels", gp.kernels_ms);
    post_device_progress(h, gp, Span{0, in.total}, in.n1);
    h->n_reads = gp.n_reads;
    return run_counting(h, gp.d_bases, gp.d_seg_off, gp.n_seg, gp.n_bases);
}

// Route 6.  The host parser (irregular framing, malformed records, SHK_HOST_PARSER=1), batch by batch.
int route_host(shk_handle *h, const Knobs &kn, const Input &in) {
    PackedReads pr;
    if (flush_every_reads(h) || in.text_total() / 2 > kn.batch_bases) h->pipe->expect_more_batches();
    if (int rc = host_parse(h, kn, in.t1, in.l1, pr, Span{0, in.total}, flush_every_reads(h))) return rc;
    if (in.fq2) if (int rc = host_parse(h, kn, in.t2, in.l2, pr, Span{in.n1, in.total}, flush_every_reads(h))) return rc;
    h->n_reads = pr.n_reads;
    h->pipe->times().add("fastq_parse_pack_host_clock", now_ms() - in.t0);
    const int rc = flush_host_batch(h, pr);
    return rc ? rc : finish_counting(h);
}

}  // namespace

int preprocess_impl(shk_handle *h, const uint8_t *fq1, size_t n1, const uint8_t *fq2, size_t n2) {
    if (!h) return SHK_E_PARAM;
    if (h->st != St::Fresh) return fail(h, SHK_E_STATE, "preprocess: handle already used (Assembler.ts:92: one preprocess per handle)");
    if (!fq1) return fail(h, SHK_E_PARAM, "preprocess: file1 is required");
    h->post_start();
    const Knobs kn;
    Input in{fq1, fq2, n1, n2, n1 + (fq2 ? n2 : 0), now_ms()};
    const bool device = !kn.host_parser;
    // .fastq.gz (the reference's real input: fastx_wasm.rs:53-70) of some size is inflated ON THE DEVICE — the compressed
    // bytes are what crosses PCIe — and its text goes straight to the device parser
    // ... unless it is a BGZF file beyond what fits at once: that is seen in the blocks' trailers before anything is uploaded
    int rc = DECLINED;
    if (device && kn.gunzip_device) {
        const int plan = plan_device_gunzip(kn, in);
        if (plan == 2) rc = route_device_bgzf_windows(h, kn, in);      // (a decline goes on below: route 1 would inflate everything to decline)
        else if (plan == 1) rc = route_device_gzip(h, kn, in);
    }
    if (rc != DECLINED) return rc;
    // whatever the device inflater does not take (several plain members, a broken BGZF chain, binary data, a damaged
    // stream) is inflated on the host (plain members: one thread per file; BGZF: block-parallel), for either parser
    std::string err;
    const uint64_t mt0 = inflate_mt_members();
    if (int ri = maybe_inflate_pair(fq1, n1, fq2, n2, in.st1, in.st2, in.t1, in.l1, in.t2, in.l2, err)) return fail_rc(h, Rc::Inflater, ri, err);
    h->pipe->times().add("gunzip_host_clock", now_ms() - in.t0);
    h->pipe->times().add("gunzip_mt_members_x1", (double)(inflate_mt_members() - mt0));     // members the multi-threaded inflater took
    const bool one_batch = in.text_total() / 2 <= kn.batch_bases;
    const bool pipelined = device && one_batch && in.text_total() >= kn.pipeline_min;
    if (pipelined) rc = route_device_pieces(h, kn, in, true);
    // (route 3 declines a text that is irregular from the first piece on: route 4 would find the same, so it is skipped)
    if (rc == DECLINED && device && one_batch && !pipelined) rc = route_device_single(h, kn, in);
    if (rc == DECLINED && device && !one_batch) rc = route_device_pieces(h, kn, in, false);
    return rc == DECLINED ? route_host(h, kn, in) : rc;
}

// ---- FASTA (shk_preprocess_fasta; SPEC S1a) ----------------------------------------------------------------------------------
// Whole files, plain or gzip, through the routes shk_preprocess has for one batch:
//   F1 fasta_device_gzip   every file is what the device inflater takes (a plain member or a BGZF chain of >= SHK_GUNZIP_DEVICE_MIN)
//                          and the text fits one batch: inflated on the device, packed there (gpu_pack_fasta), one batch
//      (what is gzip is inflated on the host here, once)
//   F2 one batch, >= SHK_FASTA_DEVICE_MIN of text: one upload, one pack on the device
//   F3 host                SHK_HOST_PARSER=1, a small text, or the device packer declined (the host packer owns the messages)
//   F4 fasta_batches       the text exceeds one batch (SHK_BATCH_BASES bytes: a FASTA byte is a base): cut on the host at header
//                          lines, each piece a batch of its own through either packer
namespace {

struct FastaBook {                                       // the counters, on every way out
    shk_handle *h; uint64_t batches0; double device = 0, host = 0;
    explicit FastaBook(shk_handle *hh) : h(hh), batches0(hh->batches_started) {}
    ~FastaBook() {
        auto &t = h->pipe->times();
        if (device) t.add("fasta_device_x1", device);
        if (host) t.add("fasta_host_x1", host);
        t.add("fasta_batches_x1", (double)(h->batches_started - batches0));
    }
};

int fasta_host_parse(shk_handle *h, const Knobs &kn, const uint8_t *t, size_t n, PackedReads &pr, const Span &sp, uint64_t flush_reads, uint64_t rec_base = 0) {
    std::string err;
    auto prog = [&](uint64_t reads, uint64_t bytes, uint64_t) { post_loop(h, reads, sp, bytes); };
    int flush_rc = SHK_OK;
    auto flush = [&](PackedReads &p) -> int { flush_rc = flush_host_batch(h, p); return flush_rc ? -7 : 0; };
    const int rc = pack_fasta(t, n, h->k, pr, err, h->progress_every(), prog, flush_reads, kn.batch_bases, flush, rec_base);
    if (rc == -7) return flush_rc;
    return rc ? fail_rc(h, Rc::Parser, rc, err) : SHK_OK;
}

int fasta_device_gzip(shk_handle *h, const Knobs &kn, const Input &in, FastaBook &book) {
    const uint8_t *gz[2] = {in.fq1, in.fq2}; const size_t gn[2] = {in.n1, in.fq2 ? in.n2 : 0};
    const int nf = in.fq2 ? 2 : 1;
    for (int f = 0; f < nf; f++) if (gn[f] < 18 || gz[f][0] != 0x1F || gz[f][1] != 0x8B) return DECLINED;
    std::string err;
    const double t0 = now_ms();
    Text text[2]; Packed packed[2];
    double ms_h2d = 0, ms_search = 0, ms_decode = 0, ms_resolve = 0;
    uint64_t bgzf_blocks = 0;
    for (int f = 0; f < nf; f++) {
        GpuInflateStats st;
        const int rc = gpu_inflate_member(gz[f], gn[f], h->pipe->device(), h->pipe->stream(), text[f], err, &st);
        if (rc == 1) { h->pipe->times().add("gunzip_device_not_taken_x1", 1.0); return DECLINED; }
        if (rc) return fail_rc(h, Rc::DeviceNoParam, rc, err);
        ms_h2d += st.h2d_ms; ms_search += st.search_ms; ms_decode += st.decode_ms; ms_resolve += st.resolve_ms;
        bgzf_blocks += st.blocks;
    }
    const double t1 = now_ms();
    Span sp;
    for (int f = 0; f < nf; f++) sp.total += text[f].e;
    if (sp.total > kn.batch_bases) return DECLINED;      // (several batches: cut on the host)
    uint64_t reads_done = 0;
    for (int f = 0; f < nf; f++) {
        const int rc = gpu_pack_fasta(nullptr, 0, nullptr, 0, h->k, h->progress_every(), h->pipe->stream(), packed[f], err, reads_done, &text[f]);
        if (rc < 0) return fail_rc(h, Rc::Device, rc, err);
        if (rc == 1) { h->pipe->times().add("fasta_device_declined_x1", 1.0); return DECLINED; }      // (inflated, but not packed: the host packer owns the message)
        reads_done += packed[f].n_reads;
        h->pipe->times().add("fasta_device_kernels", packed[f].kernels_ms);
    }
    // (marks only now that both files are packed: a decline over file 2 leaves none behind for the host route to post again)
    for (int f = 0; f < nf; f++) {
        post_device_progress(h, packed[f], sp);
        sp.base += text[f].e;
        text[f].reset();
    }
    h->pipe->times().add("gunzip_device_host_clock", t1 - t0);
    h->pipe->times().add("gunzip_device_h2d", ms_h2d);
    h->pipe->times().add("gunzip_device_search", ms_search);
    h->pipe->times().add("gunzip_device_decode", ms_decode);
    h->pipe->times().add("gunzip_device_windows_resolve_crc", ms_resolve);
    h->pipe->times().add("gunzip_device_members_x1", (double)nf);
    if (bgzf_blocks) h->pipe->times().add("gunzip_device_bgzf_blocks_x1", (double)bgzf_blocks);
    h->pipe->times().add("fasta_device_parse_pack_host_clock", now_ms() - t1);
    book.device += nf;
    h->n_reads = reads_done;
    std::vector<DevPiece> pcs;
    for (int f = 0; f < nf; f++) if (packed[f].n_seg) pcs.push_back(DevPiece{packed[f].d_bases, packed[f].d_seg_off, packed[f].n_seg, packed[f].n_bases});
    const int rc = count_pieces(h, pcs);
    return rc ? rc : finish_counting(h);
}

// F4.  Pieces of at most batch_bases bytes that begin at a header line (the first one: at the start of its file).
int fasta_batches(shk_handle *h, const Knobs &kn, const Input &in, bool device, FastaBook &book) {
    std::string err;
    const uint8_t *const text[2] = {in.t1, in.t2}; const size_t len[2] = {in.l1, in.l2};
    struct Piece { int file; size_t off, end; };
    std::vector<Piece> pieces;
    const size_t room = (size_t)kn.batch_bases;
    for (int f = 0; f < 2; f++)
        for (size_t off = 0, end; text[f] && off < len[f]; off = end) {
            end = len[f];
            if (len[f] - off > room) {
                // the last header line that begins inside (off, off + room]
                const uint8_t *t = text[f];
                size_t q = off + room + 1;                 // search t[off + 1 .. q) for a '>' behind a '\n'
                end = 0;
                while (q > off + 1) {
                    const void *g = memrchr(t + off + 1, '>', q - (off + 1));
                    if (!g) break;
                    const size_t p = (size_t)((const uint8_t *)g - t);
                    if (t[p - 1] == '\n') { end = p; break; }
                    q = p;
                }
                if (!end) {
                    const void *nx = memmem(t + off + 1, len[f] - off - 1, "\n>", 2);
                    const size_t rec_end = nx ? (size_t)((const uint8_t *)nx - t) + 1 : len[f];
                    return fail(h, SHK_E_PARAM, "preprocess_fasta: a single FASTA record of " + std::to_string(rec_end - off) +
                                " bytes exceeds one batch (SHK_BATCH_BASES = " + std::to_string(kn.batch_bases) + "): a record is never split");
                }
            }
            pieces.push_back(Piece{f, off, end});
        }
    h->pipe->expect_more_batches();
    uint64_t reads_done = 0, file_reads = 0;
    const double t0 = now_ms();
    for (size_t i = 0; i < pieces.size(); i++) {
        const Piece pc = pieces[i];
        if (i == 0 || pieces[i - 1].file != pc.file) file_reads = 0;
        const Span sp{(pc.file ? in.n1 : 0) + pc.off, in.total};
        bool on_host = !device;
        if (!on_host) {
            Packed gp;
            const int rc = gpu_pack_fasta(text[pc.file] + pc.off, pc.end - pc.off, nullptr, 0, h->k, h->progress_every(), h->pipe->stream(), gp, err, reads_done);
            if (rc < 0) return fail_rc(h, Rc::Device, rc, err);
            if (rc == 0) {
                book.device += 1;
                h->pipe->times().add("fasta_h2d_text", gp.h2d_ms);
                h->pipe->times().add("fasta_device_kernels", gp.kernels_ms);
                if (int rc2 = device_batch_in(h, gp, sp, reads_done, &file_reads)) return rc2;
            } else on_host = true;                        // declined: the host packer owns the message
        }
        if (on_host) {
            book.host += 1;
            PackedReads pr;
            pr.n_reads = reads_done;
            if (int rc = fasta_host_parse(h, kn, text[pc.file] + pc.off, pc.end - pc.off, pr, sp, flush_every_reads(h), file_reads)) return rc;
            if (int rc = flush_host_batch(h, pr)) return rc;
            file_reads += pr.n_reads - reads_done;
            reads_done = pr.n_reads;
        }
    }
    h->pipe->times().add(device ? "fasta_device_parse_pack_host_clock" : "fasta_parse_pack_host_clock", now_ms() - t0);
    h->n_reads = reads_done;
    return finish_counting(h);
}

}  // namespace

int preprocess_fasta_impl(shk_handle *h, const uint8_t *fa1, size_t n1, const uint8_t *fa2, size_t n2) {
    if (!h) return SHK_E_PARAM;
    if (h->st != St::Fresh) return fail(h, SHK_E_STATE, "preprocess_fasta: handle already used (one preprocess per handle)");
    if (!fa1) return fail(h, SHK_E_PARAM, "preprocess_fasta: file1 is required");
    h->post_start();
    const Knobs kn;
    Input in{fa1, fa2, n1, n2, n1 + (fa2 ? n2 : 0), now_ms()};
    FastaBook book(h);
    const bool device = !kn.host_parser;
    int rc = DECLINED;
    if (device && kn.gunzip_device) rc = fasta_device_gzip(h, kn, in, book);
    if (rc != DECLINED) return rc;
    std::string err;
    const uint64_t mt0 = inflate_mt_members();
    if (int ri = maybe_inflate_pair(fa1, n1, fa2, n2, in.st1, in.st2, in.t1, in.l1, in.t2, in.l2, err)) return fail_rc(h, Rc::Inflater, ri, err);
    h->pipe->times().add("gunzip_host_clock", now_ms() - in.t0);
    h->pipe->times().add("gunzip_mt_members_x1", (double)(inflate_mt_members() - mt0));
    const bool on_device = device && in.text_total() >= kn.fasta_device_min;
    if (in.text_total() > kn.batch_bases) return fasta_batches(h, kn, in, on_device, book);
    const int nf = fa2 ? 2 : 1;
    if (on_device) {
        const double t0 = now_ms();
        Packed gp;
        rc = gpu_pack_fasta(in.t1, in.l1, in.t2, in.l2, h->k, h->progress_every(), h->pipe->stream(), gp, err);
        if (rc < 0) return fail_rc(h, Rc::Device, rc, err);
        if (rc == 0) {
            book.device += nf;
            h->pipe->times().add("fasta_device_parse_pack_host_clock", now_ms() - t0);
            h->pipe->times().add("fasta_h2d_text", gp.h2d_ms);
            h->pipe->times().add("fasta_device_kernels", gp.kernels_ms);
            post_device_progress(h, gp, Span{0, in.total}, in.n1);
            h->n_reads = gp.n_reads;
            return run_counting(h, gp.d_bases, gp.d_seg_off, gp.n_seg, gp.n_bases);
        }
    }
    book.host += nf;
    PackedReads pr;
    if (flush_every_reads(h)) h->pipe->expect_more_batches();
    if (int rc2 = fasta_host_parse(h, kn, in.t1, in.l1, pr, Span{0, in.total}, flush_every_reads(h))) return rc2;
    if (fa2) if (int rc2 = fasta_host_parse(h, kn, in.t2, in.l2, pr, Span{in.n1, in.total}, flush_every_reads(h))) return rc2;
    h->n_reads = pr.n_reads;
    h->pipe->times().add("fasta_parse_pack_host_clock", now_ms() - in.t0);
    rc = flush_host_batch(h, pr);
    return rc ? rc : finish_counting(h);
}

int push_reads_impl(shk_handle *h, const uint8_t *chunk, size_t n) {
    if (!h) return SHK_E_PARAM;
    if (h->st != St::Fresh && h->st != St::Streaming) return fail(h, SHK_E_STATE, "push_reads: handle already preprocessed");
    if (h->st == St::Fresh) {
        h->post_start();
        h->st = St::Streaming;
    }
    const Knobs kn;
    const Span no_pct{0, 0, false};
    h->pipe->expect_more_batches();                      // the total is unknown while chunks keep coming
    // a large chunk (whole records, like every chunk) is parsed on the device and counted as a batch of its
    // own; small chunks — and any chunk the device parser finds irregular — are packed on the host below
    if (!kn.host_parser && n >= kn.stream_device_min) {
        std::string err;
        ByteVec st;
        const uint8_t *t = nullptr; size_t l = 0;
        int rc = maybe_inflate(chunk, n, st, t, l, err);
        if (rc) return fail_rc(h, Rc::Inflater, rc, err);
        if (l / 2 <= kn.batch_bases) {
            Packed gp;
            rc = gpu_pack_fastq(t, l, nullptr, 0, h->k, h->min_qual, h->progress_every(), h->pipe->stream(), gp, err, h->stream_reads.n_reads);
            if (rc < 0) return fail_rc(h, Rc::Device, rc, err);
            if (rc == 0) {
                h->pipe->times().add("fastq_device_chunks_x1", 1.0);
                h->stream_reads.n_input_bases += gp.n_input_bases;
                return device_batch_in(h, gp, no_pct, h->stream_reads.n_reads);
            }
            // (rc == 1, not regular 4-line FASTQ: the host parser decides)
        }
    }
    return host_parse(h, kn, chunk, n, h->stream_reads, no_pct, flush_every_reads(h));
}

int finish_reads_impl(shk_handle *h) {
    if (!h) return SHK_E_PARAM;
    if (h->st != St::Streaming) return fail(h, SHK_E_STATE, "finish_reads: no reads pushed");
    h->n_reads = h->stream_reads.n_reads;
    int rc = flush_host_batch(h, h->stream_reads);
    h->stream_reads.clear();
    return rc ? rc : finish_counting(h);
}

int preprocess_packed_device_impl(shk_handle *h, const void *d_bases, const void *d_seg_off, uint64_t n_seg,
                                  uint64_t n_bases, uint64_t n_reads) {
    if (!h) return SHK_E_PARAM;
    if (h->st != St::Fresh) return fail(h, SHK_E_STATE, "preprocess: handle already used");
    if (!d_bases || !d_seg_off) return fail(h, SHK_E_PARAM, "null device pointer");
    h->post_start();
    h->n_reads = n_reads;
    h->post_mode(("loop:" + std::to_string(n_reads) + ":100").c_str());
    return run_counting(h, (const uint32_t *)d_bases, (const uint32_t *)d_seg_off, n_seg, n_bases);
}

int preprocess_packed_host_impl(shk_handle *h, const uint32_t *bases, const uint32_t *seg_off, uint64_t n_seg,
                                uint64_t n_bases, uint64_t n_reads) {
    if (h->st != St::Fresh) return fail(h, SHK_E_STATE, "preprocess: handle already used");
    if (!bases || !seg_off) return fail(h, SHK_E_PARAM, "null host pointer");
    if (n_bases >= 0xFFFFFFFFull || n_seg >= 0xFFFFFFFFull) return fail(h, SHK_E_PARAM, "batch too large (>= 2^32 bases)");
    std::string err;
    const size_t want_b = (size_t)((n_bases + 15) / 16 + 1) * 4, want_s = (size_t)(n_seg + 1) * 4;
    void *st = h->pipe->stream();
    double t0 = 0;
    int rc = 0;
    {   // (the scope ends in front of the host-clock total: its drain is part of the figure)
        PoolScope sc(st);                                      // the blocks go back to the pool idle, also after a failure
        uint32_t *db = sc.get<uint32_t>(want_b / 4, err), *ds = sc.get<uint32_t>(want_s / 4, err);
        if (!db || !ds) return fail(h, SHK_E_OOM, "preprocess: device memory for the packed reads");
        t0 = now_ms();
        h->post_start();
        h->n_reads = n_reads;
        h->post_mode(("loop:" + std::to_string(n_reads) + ":100").c_str());
        // upload and pass 1 overlap piece by piece (Pipeline::count_batch_host), then histogram / fit / filter as usual
        h->batches_started++;
        h->pipe->single_batch_resident(true);
        rc = h->pipe->count_batch_host(db, ds, bases, seg_off, n_seg, n_bases, err);
        if (rc) rc = fail_rc(h, Rc::Device, rc, err);
        else rc = finish_counting(h);
        h->pipe->single_batch_resident(false);
    }
    h->pipe->times().add("h2d_packed_reads_MB", (double)(want_b + want_s) / 1e6);
    h->pipe->times().add("preprocess_from_host_total_host_clock", now_ms() - t0);
    return rc;
}
