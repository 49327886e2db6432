// shard_preprocess.cpp — the sharded preprocess (DESIGN.md "Multi-GPU"): the single-GPU preprocess cut at its two exchange
// points (the shard_*_impl steps, which a caller with collectives of its own drives too), and the collective call that runs
// them between the library's own collectives (shard_comm.h), one sp_* function per step over one ShardPrep.  What the host
// decides between the steps — the size row, the dedupe verdict, the byte layouts — is exchange_plan.h's.
//
// A failure on ONE rank (device memory, a slice that overflows, a partition beyond 2^32 records: all depend on that rank's
// share of the reads) must not leave the others blocked in the next collective: every local step's result travels with the
// next small collective — as an extra word of one that exists anyway (`carried`), or as a one-word all-reduce in front of
// the two big exchanges (`agree`) — and all ranks leave together.  A collective that fails itself marks the communicator
// broken (shk_comm_free then aborts it: peers fail fast).
#include "shard_preprocess.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <functional>
#include <vector>

#include "preprocess.h"

namespace shk { bool spectrum_fit(const uint64_t *histo500, uint32_t *out); }   // fit.cpp

using namespace shk;

// ---- the steps of the public step API ---------------------------------------------------------------------------------------

int shard_partition_impl(shk_handle *h, const void *d_bases, const void *d_seg_off, uint64_t n_seg, uint64_t n_bases,
                         uint64_t n_reads, uint32_t n_partitions, uint64_t *part_records) {
    if (!h || !part_records) return SHK_E_PARAM;
    if (h->st != St::Fresh) return fail(h, SHK_E_STATE, "shard_partition: handle already used");
    h->post_start();
    h->n_reads = n_reads;
    std::vector<uint64_t> pr;
    std::string err;
    int rc = h->pipe->shard_partition((const uint32_t *)d_bases, (const uint32_t *)d_seg_off, n_seg, n_bases, n_partitions, pr, err);
    if (rc) return fail_rc(h, Rc::Device, rc, err);
    memcpy(part_records, pr.data(), (size_t)n_partitions * 8);
    h->post_mode(("loop:" + std::to_string(n_reads) + ":100").c_str());
    h->post_loop_edge("loop:end");
    h->st = St::Sharding;
    return SHK_OK;
}

int shard_pack_impl(shk_handle *h, void *d_send, const uint64_t *base_records, uint32_t n_partitions) {
    if (!h || !base_records) return SHK_E_PARAM;
    if (h->st != St::Sharding) return fail(h, SHK_E_STATE, "shard_pack: call shard_partition first");
    std::string err;
    int rc = h->pipe->shard_pack(d_send, base_records, n_partitions, err);
    return rc ? fail_rc(h, Rc::Device, rc, err) : SHK_OK;
}

int shard_count_impl(shk_handle *h, const void *d_recv, const uint64_t *run_off, const uint32_t *run_cnt, uint32_t n_owned,
                     uint32_t n_sources, uint64_t *histo500_local, uint64_t *n_instances_local, const void *d_recv_w) {
    if (!h || !histo500_local) return SHK_E_PARAM;
    if (h->st != St::Sharding) return fail(h, SHK_E_STATE, "shard_count: call shard_partition first");
    std::string err;
    if (!h->do_bloom && h->chunk_size == 0) h->post("preprocess:bulk:sorting");
    int rc = h->pipe->shard_count(d_recv, d_recv_w, run_off, run_cnt, n_owned, n_sources, emit_threshold_of(h), histo500_local, err);
    if (rc) return fail_rc(h, Rc::Device, rc, err);
    if (n_instances_local) *n_instances_local = h->pipe->total_instances();
    return SHK_OK;
}

int shard_rows_impl(shk_handle *h, const uint64_t *histo500_global, const void **d_keys, const void **d_cnt, uint64_t *n_rows,
                    uint32_t *used_min_count) {
    if (!h || !histo500_global || !d_keys || !d_cnt || !n_rows) return SHK_E_PARAM;
    if (h->st != St::Sharding) return fail(h, SHK_E_STATE, "shard_rows: call shard_count first");
    memcpy(h->histo, histo500_global, sizeof h->histo);
    h->used_min_count = h->min_count; h->fit_ok = false;
    if (h->do_fit) {
        h->post_mode("fitting");
        uint32_t v = 0;
        if (spectrum_fit(h->histo, &v)) { h->used_min_count = v; h->fit_ok = true; }
    }
    h->post_mode("filtering");
    std::string err;
    int rc = h->pipe->shard_rows(h->used_min_count, d_keys, d_cnt, n_rows, err);
    if (rc) return fail_rc(h, Rc::DeviceNoParam, rc, err);
    if (used_min_count) *used_min_count = h->used_min_count;
    return SHK_OK;
}

int shard_set_solid_impl(shk_handle *h, const void *const *d_keys, const void *d_cnt, uint64_t n_rows, uint64_t n_instances_global) {
    if (!h) return SHK_E_PARAM;
    if (h->st != St::Sharding) return fail(h, SHK_E_STATE, "shard_set_solid: call shard_rows first");
    std::string err;
    int rc = h->pipe->shard_set_solid(d_keys, d_cnt, n_rows, h->histo, n_instances_global, err);
    if (rc) return fail_rc(h, Rc::Device, rc, err);
    h->post("preprocess:saving");
    h->pre_json = preprocessing_json(h->pipe->n_solid(), h->histo, h->used_min_count);
    h->st = St::Preprocessed;
    h->post("preprocess:end");
    return SHK_OK;
}

// ---- the collective call ----------------------------------------------------------------------------------------------------

namespace {

// This rank's reads as shard_preprocess_impl takes them: a step that hands over any number of batches (none, one, several: the
// ranks need not agree), each of which goes through pass 1 at once and is the step's again afterwards.
//   inst_ub   the k-mer instances of all the batches — n_bases - n_seg * (k - 1) summed — where the rank knows them before it
//             starts (packed reads), else an upper bound (files read window by window: text bytes / 2).  What the rank adds to
//             the instance all-reduce from which P is chosen (n_partitions == 0): pass 1 of the FIRST batch needs P.
//   feed      calls sink.batch once per batch; SHK_OK, or the code of an error that is set in the handle (a failure in a later
//             batch travels with the size exchange, as every failure of pass 1 does)
//   n_reads   where feed does not count them itself (it then leaves h->n_reads to the sink's last batch)
struct ShardReads {
    uint64_t inst_ub = 0, n_reads = 0;
    std::function<int(ShardBatchSink &)> feed;
};
uint64_t instances_of(const shk_handle *h, uint64_t n_seg, uint64_t n_bases) {
    return n_bases > n_seg * (uint64_t)(h->k - 1) ? n_bases - n_seg * (uint64_t)(h->k - 1) : 0;
}

// pass 1 batch by batch: every batch into the same P partitions (Pipeline::shard_add_batch), one progress string each
struct Sink : ShardBatchSink {
    shk_handle *h; uint64_t n_batches = 0, inst = 0, last_pct = 0;
    explicit Sink(shk_handle *hh) : h(hh) {}
    int batch(const uint32_t *d_bases, const uint32_t *d_seg_off, uint64_t n_seg, uint64_t n_bases, uint64_t n_reads, uint64_t text_done,
              uint64_t text_total) override {
        std::string e2;
        if (int rc = h->pipe->shard_add_batch(d_bases, d_seg_off, n_seg, n_bases, e2)) return fail_rc(h, Rc::Device, rc, e2);
        n_batches++;
        inst += instances_of(h, n_seg, n_bases);
        h->n_reads = n_reads;
        last_pct = text_total ? std::min<uint64_t>(100, std::max<uint64_t>(last_pct, (uint64_t)((unsigned __int128)100 * text_done / text_total))) : 100;
        h->post_mode(("loop:" + std::to_string(n_reads) + ":" + std::to_string(last_pct)).c_str());
        return SHK_OK;
    }
};

// SHK_FAULT_INJECT=<step> (read — the entry points from files alone — | pass1 | pack | count | rows | keep | alloc) makes that
// local step of THIS process fail: the tests set it on one rank to see every rank leave with an error instead of hanging.  It
// never changes a result.
int injected(shk_handle *h, const char *step) {
    const char *inject = getenv("SHK_FAULT_INJECT");
    return (inject && !strcmp(inject, step)) ? fail(h, SHK_E_INTERNAL, std::string("injected fault (SHK_FAULT_INJECT=") + step + ")") : SHK_OK;
}
std::string peer_failed_msg(const char *stage) {
    return std::string("shard_preprocess: another rank failed during ") + stage + " (this rank's state is intact up to there; free the handle)";
}
// The one-word all-reduce of "I failed".  This rank's own failure first (its code, its message in the handle); else the
// collective's; else SHK_E_DEVICE with peer_msg where another rank's flag was set.
int agree(shk_handle *h, ShardComm *c, void *st, int local_rc, const std::string &peer_msg) {
    uint64_t f = local_rc ? 1u : 0u;
    std::string e2;
    if (int rc = comm_allreduce_host_u64(c, &f, 1, st, e2)) return local_rc ? local_rc : fail_rc(h, Rc::Device, rc, e2);
    if (local_rc) return local_rc;
    return f ? fail(h, SHK_E_DEVICE, peer_msg) : SHK_OK;
}

// Everything one shard_preprocess call owns.  THE RULE (as at Pipeline's ShardRun): the PoolScope is the LAST member, so it is
// the first to go — on every way out, errors included, the stream is drained, through the watchdog, before a block goes back
// to the pool and before any host vector a step filled is freed.
struct ShardPrep {
    shk_handle *h; ShardComm *c; void *st;
    uint32_t world, rank, W, P = 0;
    const double t0 = now_ms();
    const bool stage_log = getenv("SHK_STAGE_LOG") != nullptr;      // (see stage)
    std::string err;                                      // of the collective that failed
    Sink sink;
    int rc_p1 = SHK_OK;                                   // what pass 1 returned: travels with the size exchange
    std::vector<uint64_t> row, rows;                      // this rank's size row (exchange_plan.h); the gathered rows
    DedupeVerdict v;                                      // v.weighted: distinct records + u32 weights travel
    ExchangePlan plan;
    ExchangeBytes xb;                                     // the record exchange in bytes
    uint64_t rec_bytes = 0;
    uint8_t *send = nullptr, *recv = nullptr, *send_w = nullptr, *recv_w = nullptr;
    uint64_t red[SHK_HISTO_BINS + HT_WORDS] = {0};        // the histogram, then the HistoTail words: this rank's, then reduced
    const void *keys[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}; const void *cnt = nullptr;      // this rank's solid rows
    uint64_t n_local = 0;
    int rc_rows = SHK_OK;                                 // what the filter returned: travels with the rows all-gather
    std::vector<uint64_t> counts;                         // solid rows per rank
    PoolScope sc;

    ShardPrep(shk_handle *hh, ShardComm *cc)
        : h(hh), c(cc), st(hh->pipe->stream()), world((uint32_t)comm_world(cc)), rank((uint32_t)comm_rank(cc)), W((2 * hh->k + 63) / 64),
          sink(hh), sc([cc, s = hh->pipe->stream()] { std::string e; (void)comm_stream_wait(cc, s, e); }) {}

    // SHK_STAGE_LOG=1: after every step the stream is drained and the step's name goes to stderr (which step a fault belongs to)
    void stage(const char *what) const {
        if (!stage_log) return;
        std::string e2; const int r2 = device_stream_sync(st, e2);
        fprintf(stderr, "[shard_preprocess rank %u] %s done%s\n", rank, what, r2 ? " (stream error)" : ""); fflush(stderr);
    }
    // "This collective carried my flag": coll_rc is what the collective returned (its message in err), peer_flag whether a
    // flag was set in what it delivered.  This rank's own failure first, then the collective's, then the other rank's.
    int carried(int local_rc, int coll_rc, bool peer_flag, const char *stage_name) {
        if (local_rc) return local_rc;
        if (coll_rc) return fail_rc(h, Rc::Device, coll_rc, err);
        return peer_flag ? fail(h, SHK_E_DEVICE, peer_failed_msg(stage_name)) : SHK_OK;
    }
    int agree(int local_rc, const char *stage_name) { return ::agree(h, c, st, local_rc, peer_failed_msg(stage_name)); }
};

// ---- 1. the partition count must be the same everywhere: from the global instance count
int sp_choose_partitions(ShardPrep &s, const ShardReads &reads, uint32_t n_partitions) {
    if (n_partitions == 0) {
        uint64_t inst = reads.inst_ub;
        if (int rc = comm_allreduce_host_u64(s.c, &inst, 1, s.st, s.err)) return fail_rc(s.h, Rc::Device, rc, s.err);
        n_partitions = choose_partitions(inst, s.world, s.W == 1 ? 100000 : 40000);
    }
    if (n_partitions < s.world) return fail(s.h, SHK_E_PARAM, "shard_preprocess: fewer partitions than ranks");
    s.P = n_partitions;
    return SHK_OK;
}

// ---- 2. pass 1 on this rank's reads, then the records are deduplicated HERE, before they cross the fabric (at 100x a
// super-k-mer record recurs ~50 times; count_part.h: k_dedupe_partitions): distinct records + u32 weights travel.
// SHK_SHARD_DEDUPE: 0 = never, 1 = always, default = when the distinct records of all ranks are at most half of the raw
// ones (error-rich reads do not deduplicate, and their partitions need the k-mer-level repartition, which counts
// unweighted records).  Bloom mode counts raw records too.  The decision is taken from the gathered rows: same everywhere.
// No way out: what the step returned (s.rc_p1) travels with the size row.
void sp_pass1(ShardPrep &s, const ShardReads &reads) {
    shk_handle *h = s.h;
    const uint32_t P = s.P;
    std::vector<uint64_t> send(P, 0), raw(P, 0);
    uint64_t mode = DEDUPE_RAW;
    int &rc = s.rc_p1;
    h->post_start();
    h->n_reads = reads.n_reads;
    { std::string e2; if (int r2 = h->pipe->shard_begin(P, e2)) rc = fail_rc(h, Rc::Device, r2, e2); }
    if (!rc) rc = reads.feed(s.sink);
    if (!rc) {
        std::vector<uint64_t> pr; std::string e2;
        if (int r2 = h->pipe->shard_totals(pr, e2)) rc = fail_rc(h, Rc::Device, r2, e2);
        else std::copy_n(pr.begin(), P, send.begin());
    }
    if (!rc) {
        if (s.sink.n_batches == 0 || s.sink.last_pct != 100) h->post_mode(("loop:" + std::to_string(h->n_reads) + ":100").c_str());
        h->post_loop_edge("loop:end");
        h->st = St::Sharding;
    }
    if (!rc) rc = injected(h, "pass1");
    if (!rc) {
        raw = send;
        const char *dd = getenv("SHK_SHARD_DEDUPE");
        mode = (dd && *dd == '0') || h->do_bloom ? DEDUPE_RAW : ((dd && *dd == '1') ? DEDUPE_ALWAYS : DEDUPE_AUTO);
        if (mode != DEDUPE_RAW) {
            std::vector<uint64_t> pr(send);
            std::string e2;
            if (int r2 = h->pipe->shard_dedupe(pr, e2)) rc = fail_rc(h, Rc::DeviceNoParam, r2, e2);
            else std::copy_n(pr.begin(), P, send.begin());
        }
    }
    s.row = size_row_fill(P, send.data(), raw.data(), rc != SHK_OK, mode);
    s.stage("pass 1 + dedupe");
}

// ---- 3. the size exchange: every rank learns what every rank holds per partition; the verdict on the weights
int sp_size_exchange(ShardPrep &s) {
    s.rows.assign((size_t)s.world * s.row.size(), 0);
    const int rc = comm_allgather_host_u64(s.c, s.row.data(), s.row.size(), s.rows.data(), s.st, s.err);
    if (!rc && !s.rc_p1) s.v = dedupe_verdict(s.rows, s.world, s.P);
    if (int out = s.carried(s.rc_p1, rc, s.v.peer_failed, "pass 1")) return out;
    if (!s.v.weighted) s.h->pipe->shard_drop_dedup();
    s.h->pipe->times().add("shard_records_deduplicated_x1", s.v.weighted ? 1.0 : 0.0);
    s.rec_bytes = (uint64_t)s.h->pipe->rec_words() * 8u;
    return SHK_OK;
}

// ---- 4. pack (destination-major); the ranks agree that all of them have packed
int sp_pack(ShardPrep &s) {
    shk_handle *h = s.h;
    const DedupeVerdict &v = s.v;
    int rc_pack = SHK_OK;
    if (int rc = plan_exchange(v.counts.data(), s.world, s.P, s.rank, s.plan, s.err)) rc_pack = fail_rc(h, Rc::Device, rc, s.err);
    if (!rc_pack && !raw_records_fit(v, s.world, s.P, s.rank)) rc_pack = fail(h, SHK_E_PARAM, "a partition holds more than 2^32 records");
    if (!rc_pack) {
        s.xb = exchange_bytes(s.plan, s.rec_bytes);
        std::string e2;
        s.send = s.sc.get<uint8_t>((size_t)(s.xb.n_send * s.rec_bytes + 64), e2);
        s.recv = s.sc.get<uint8_t>((size_t)(s.xb.n_recv * s.rec_bytes + 64), e2);
        if (s.v.weighted) {
            s.send_w = s.sc.get<uint8_t>((size_t)(s.xb.n_send * 4 + 64), e2);
            s.recv_w = s.sc.get<uint8_t>((size_t)(s.xb.n_recv * 4 + 64), e2);
        }
        if (!s.send || !s.recv || (s.v.weighted && (!s.send_w || !s.recv_w))) rc_pack = fail(h, SHK_E_OOM, "shard_preprocess: device memory for the record exchange");
    }
    if (!rc_pack && s.v.weighted) {
        std::string e2;
        if (int r2 = h->pipe->shard_pack_dedup(s.send, s.send_w, s.plan.base.data(), s.P, e2)) rc_pack = fail_rc(h, Rc::Device, r2, e2);
    } else if (!rc_pack) rc_pack = shard_pack_impl(h, s.send, s.plan.base.data(), s.P);
    if (!rc_pack) rc_pack = injected(h, "pack");
    s.stage("pack");
    return s.agree(rc_pack, "the packing of the records");
}

// ---- 5. the exchange: the records, then their weights (the same element offsets, 4 bytes each)
int sp_exchange(ShardPrep &s) {
    shk_handle *h = s.h;
    const ExchangeBytes &x = s.xb;
    const double tx = now_ms();
    if (int rc = comm_alltoallv(s.c, s.send, x.send_off.data(), x.send_bytes.data(), s.recv, x.recv_off.data(), x.recv_bytes.data(), s.st, s.err))
        return fail_rc(h, Rc::Device, rc, s.err);
    if (s.v.weighted) {
        const ExchangeBytes w = exchange_bytes(s.plan, 4);
        if (int rc = comm_alltoallv(s.c, s.send_w, w.send_off.data(), w.send_bytes.data(), s.recv_w, w.recv_off.data(), w.recv_bytes.data(), s.st, s.err, 4))
            return fail_rc(h, Rc::Device, rc, s.err);
    }
    if (int rc = comm_stream_wait(s.c, s.st, s.err)) { comm_mark_broken(s.c); return fail_rc(h, Rc::Device, rc, s.err); }
    h->pipe->times().add("shard_exchange_host_clock", now_ms() - tx);
    h->pipe->times().add("shard_exchange_sent_MB", (double)(x.n_send * (s.rec_bytes + (s.v.weighted ? 4 : 0))) / 1e6);
    s.stage("exchange");
    s.sc.release(s.send_w); s.send_w = nullptr;          // (the stream is idle: the wait above)
    s.sc.release(s.send); s.send = nullptr;
    return SHK_OK;
}

// ---- 6. pass 2 over the owned partitions, then the global histogram with the HistoTail words behind it
int sp_count(ShardPrep &s) {
    uint64_t *tail = &s.red[SHK_HISTO_BINS];
    int rc_cnt = shard_count_impl(s.h, s.recv, s.plan.run_off.data(), s.plan.run_cnt.data(), (uint32_t)s.plan.owned.size(), s.world, s.red,
                                  &tail[HT_COUNTED], s.v.weighted ? s.recv_w : nullptr);
    s.stage("pass 2");
    if (!rc_cnt) rc_cnt = injected(s.h, "count");
    if (rc_cnt) memset(s.red, 0, sizeof s.red);
    tail[HT_FAILED] = rc_cnt ? 1u : 0u;
    tail[HT_IN_READS] = s.sink.inst;                      // (summed over this rank's batches)
    const int rc = comm_allreduce_host_u64(s.c, s.red, SHK_HISTO_BINS + HT_WORDS, s.st, s.err);
    if (int out = s.carried(rc_cnt, rc, tail[HT_FAILED] != 0, "pass 2")) return out;
    const std::string lost = instances_mismatch(tail);
    return lost.empty() ? SHK_OK : fail(s.h, SHK_E_INTERNAL, lost);
}

// SHK_STAGE_LOG (debug aid): are the rank's solid k-mers distinct?
void print_duplicate_kmers(const ShardPrep &s) {
    const uint64_t n_local = s.n_local; const uint32_t W = s.W, rank = s.rank;
    std::vector<std::vector<uint64_t>> kw(W, std::vector<uint64_t>(n_local));
    bool ok = true;
    for (uint32_t j = 0; j < W && ok; j++) { void *dp = const_cast<void *>(s.keys[j]); std::string e3; ok = device_download(kw[j].data(), dp, n_local * 8, e3) == 0; }
    if (!ok) return;
    std::vector<uint32_t> idx(n_local);
    for (uint32_t i = 0; i < n_local; i++) idx[i] = i;
    std::sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { for (int j = (int)W - 1; j >= 0; j--) if (kw[j][a] != kw[j][b]) return kw[j][a] < kw[j][b]; return false; });
    uint64_t dup = 0;
    for (uint32_t i = 1; i < n_local; i++) {
        bool eq = true; for (uint32_t j = 0; j < W; j++) eq = eq && kw[j][idx[i]] == kw[j][idx[i - 1]];
        if (eq && dup < 4) fprintf(stderr, "[shard_preprocess rank %u]   duplicate k-mer %016llx at rows %u and %u\n", rank, (unsigned long long)kw[0][idx[i]], idx[i - 1], idx[i]);
        dup += eq;
    }
    fprintf(stderr, "[shard_preprocess rank %u] %llu local solid k-mers, %llu duplicates\n", rank, (unsigned long long)n_local, (unsigned long long)dup); fflush(stderr);
}

// ---- 7. fit / filter (identical on every rank), local solid rows.  No way out: s.rc_rows travels with the row counts.
void sp_rows(ShardPrep &s) {
    uint32_t used = 0;
    s.rc_rows = shard_rows_impl(s.h, s.red, s.keys, &s.cnt, &s.n_local, &used);
    s.stage("filter");
    if (s.stage_log && !s.rc_rows && s.n_local && s.n_local < (1u << 24)) print_duplicate_kmers(s);
    if (!s.rc_rows) s.rc_rows = injected(s.h, "rows");
}

// ---- 8. all-gather of the row counts, {rows, this rank failed} each
int sp_rows_gather(ShardPrep &s) {
    std::vector<uint64_t> counts2((size_t)s.world * 2);
    const uint64_t mine2[2] = {s.rc_rows ? 0u : s.n_local, s.rc_rows ? 1u : 0u};
    const int rc = comm_allgather_host_u64(s.c, mine2, 2, counts2.data(), s.st, s.err);
    bool peer = false;
    s.counts.assign(s.world, 0);
    for (uint32_t r = 0; r < s.world && !rc; r++) { peer = peer || counts2[2 * r + 1]; s.counts[r] = counts2[2 * r]; }
    return s.carried(s.rc_rows, rc, peer, "the filter");
}

// ---- 9. the graph stays sharded (default): every rank keeps its own rows and shk_assemble() runs collectively over this
// communicator (csrc/shard_graph.h)
int sp_keep_local(ShardPrep &s) {
    shk_handle *h = s.h;
    int rc_keep = SHK_OK;
    { std::string e2; const int r2 = h->pipe->shard_keep_local(s.world, s.rank, s.P, s.counts.data(), s.red, s.red[SHK_HISTO_BINS + HT_COUNTED], e2);
      if (r2) rc_keep = fail(h, r2 == -1 ? SHK_E_PARAM : SHK_E_DEVICE, e2); }
    if (!rc_keep) rc_keep = injected(h, "keep");
    if (int rc = s.agree(rc_keep, "the hand-over to the sharded assembly")) return rc;
    h->shard_comm = s.c;
    h->post("preprocess:saving");
    h->pre_json = preprocessing_json(h->pipe->n_solid_global(), h->histo, h->used_min_count);
    h->st = St::Preprocessed;
    h->post("preprocess:end");
    h->pipe->times().add("shard_preprocess_host_clock", now_ms() - s.t0);
    return SHK_OK;
}

// ---- 9'. SHK_SHARD_GRAPH=0: round 2's path — gather the solid set, assemble on every rank
int sp_gather_solid(ShardPrep &s) {
    shk_handle *h = s.h;
    const GatherLayout g = gather_layout(s.counts);
    uint8_t *gk[8] = {}, *gc = nullptr;
    int rc_alloc = SHK_OK;
    for (uint32_t j = 0; j < s.W && !rc_alloc; j++) {
        std::string e2;
        gk[j] = s.sc.get<uint8_t>((size_t)(g.n_total * 8 + 64), e2);
        if (!gk[j]) rc_alloc = fail(h, SHK_E_OOM, "shard_preprocess: device memory for the solid set");
    }
    if (!rc_alloc) {
        std::string e2;
        gc = s.sc.get<uint8_t>((size_t)(g.n_total * 4 + 64), e2);
        if (!gc) rc_alloc = fail(h, SHK_E_OOM, "shard_preprocess: device memory for the solid set");
    }
    if (!rc_alloc) rc_alloc = injected(h, "alloc");
    if (int rc = s.agree(rc_alloc, "the allocation of the solid set")) return rc;
    for (uint32_t j = 0; j < s.W; j++)
        if (int rc = comm_allgatherv(s.c, s.keys[j], gk[j], g.off8.data(), g.len8.data(), s.st, s.err)) return fail_rc(h, Rc::Device, rc, s.err);
    if (int rc = comm_allgatherv(s.c, s.cnt, gc, g.off4.data(), g.len4.data(), s.st, s.err)) return fail_rc(h, Rc::Device, rc, s.err);
    if (int rc = comm_stream_wait(s.c, s.st, s.err)) { comm_mark_broken(s.c); return fail_rc(h, Rc::Device, rc, s.err); }
    const void *kp[8] = {gk[0], gk[1], gk[2], gk[3], gk[4], gk[5], gk[6], gk[7]};
    if (int rc = shard_set_solid_impl(h, kp, gc, g.n_total, s.red[SHK_HISTO_BINS + HT_COUNTED])) return rc;
    h->pipe->times().add("shard_preprocess_host_clock", now_ms() - s.t0);
    return SHK_OK;
}

int shard_preprocess_impl(shk_handle *h, shk_comm *cm, const ShardReads &reads, uint32_t n_partitions) {
    if (!cm || !cm->c) return fail(h, SHK_E_PARAM, "shard_preprocess: null communicator");
    if (h->st != St::Fresh) return fail(h, SHK_E_STATE, "shard_preprocess: handle already used");
    if (comm_device(cm->c) != h->pipe->device()) return fail(h, SHK_E_PARAM, "shard_preprocess: communicator and handle live on different devices");
    ShardPrep s(h, cm->c);
    if (int rc = sp_choose_partitions(s, reads, n_partitions)) return rc;
    sp_pass1(s, reads);
    if (int rc = sp_size_exchange(s)) return rc;
    if (int rc = sp_pack(s)) return rc;
    if (int rc = sp_exchange(s)) return rc;
    if (int rc = sp_count(s)) return rc;
    sp_rows(s);
    if (int rc = sp_rows_gather(s)) return rc;
    const char *sg = getenv("SHK_SHARD_GRAPH");
    return (sg && *sg == '0') ? sp_gather_solid(s) : sp_keep_local(s);
}

// one batch that lies in HBM already
ShardReads one_batch(shk_handle *h, const void *d_bases, const void *d_seg_off, uint64_t n_seg, uint64_t n_bases, uint64_t n_reads) {
    ShardReads r;
    r.inst_ub = instances_of(h, n_seg, n_bases);
    r.n_reads = n_reads;
    r.feed = [=](ShardBatchSink &sink) { return sink.batch((const uint32_t *)d_bases, (const uint32_t *)d_seg_off, n_seg, n_bases, n_reads, 1, 1); };
    return r;
}

// several (shk_shard_preprocess_batches): the reads posted with a batch are n_reads in proportion to the bases so far
int preprocess_batches(shk_handle *h, shk_comm *cm, uint32_t n_batches, const void *const *d_bases, const void *const *d_seg_off,
                       const uint64_t *n_seg, const uint64_t *n_bases, uint64_t n_reads, uint32_t n_partitions) {
    if (n_batches && (!d_bases || !d_seg_off || !n_seg || !n_bases)) return fail(h, SHK_E_PARAM, "shard_preprocess_batches: null batch arrays");
    if (n_batches == 1) return shard_preprocess_impl(h, cm, one_batch(h, d_bases[0], d_seg_off[0], n_seg[0], n_bases[0], n_reads), n_partitions);
    ShardReads r;
    uint64_t total_bases = 0;
    for (uint32_t b = 0; b < n_batches; b++) {
        if (n_seg[b] && (!d_bases[b] || !d_seg_off[b])) return fail(h, SHK_E_PARAM, "shard_preprocess_batches: a batch with segments and no memory");
        r.inst_ub += instances_of(h, n_seg[b], n_bases[b]);
        total_bases += n_bases[b];
    }
    r.n_reads = n_reads;
    r.feed = [=](ShardBatchSink &sink) {
        uint64_t bases = 0;
        for (uint32_t b = 0; b < n_batches; b++) {
            bases += n_bases[b];
            const uint64_t so_far = b + 1 == n_batches || !total_bases ? n_reads : (uint64_t)((unsigned __int128)n_reads * bases / total_bases);
            if (int rc = sink.batch((const uint32_t *)d_bases[b], (const uint32_t *)d_seg_off[b], n_seg[b], n_bases[b], so_far, b + 1, n_batches)) return rc;
        }
        return (int)SHK_OK;
    };
    return shard_preprocess_impl(h, cm, r, n_partitions);
}

// shk_shard_preprocess from FASTQ files.  A share that fits one batch is read into ONE packed batch in HBM (share_reader.cpp:
// read_fastq_share — split: slice `rank` of `world` of the same files on every rank; else the rank's own files, whole), the
// ranks agree that all of them have their reads, and the batch goes through shard_preprocess_impl as it is.  A larger share is
// only looked at in front of that agreement (read_fastq_share says in_batches before it uploads anything, where it can) and is
// read inside pass 1, window by window (read_fastq_share_batches): its failures travel with the size exchange.
int preprocess_files(shk_handle *h, shk_comm *cm, const uint8_t *fq1, size_t n1, const uint8_t *fq2, size_t n2, uint32_t n_partitions, int split,
                     RecFmt fmt) {
    // (FASTA, shk_shard_preprocess_fasta: the same steps — the readers take the format; its names in the messages and the timings)
    const bool fasta = fmt == RecFmt::Fasta;
    const std::string entry = fasta ? "shard_preprocess_fasta" : "shard_preprocess_fastq", tag = fasta ? "shard_fasta_" : "shard_fastq_";
    if (!cm || !cm->c) return fail(h, SHK_E_PARAM, entry + ": null communicator");
    if (h->st != St::Fresh) return fail(h, SHK_E_STATE, entry + ": handle already used");
    if (comm_device(cm->c) != h->pipe->device()) return fail(h, SHK_E_PARAM, entry + ": communicator and handle live on different devices");
    ShardComm *c = cm->c;
    void *st = h->pipe->stream();
    const double t0 = now_ms();
    FastqShare sh;
    // (declared after the share: its blocks go back to the pool with the stream idle, on every way out)
    struct DrainOnExit { void *st; ~DrainOnExit() { std::string e; (void)device_stream_sync(st, e); } } drain{st};
    // A rank whose reading fails (a parse error, a damaged stream, memory) enters the first collective all the same, with
    // "I failed": it returns its own code and message, every other rank "another rank failed during reading".
    std::string err;
    const uint32_t s_rank = split ? (uint32_t)comm_rank(c) : 0u, s_world = split ? (uint32_t)comm_world(c) : 1u;
    int rc_read = read_fastq_share(fq1, n1, fq2, n2, h->k, h->min_qual, s_rank, s_world, h->pipe->device(), st, sh, err, true, fmt);
    if (rc_read) rc_read = fail(h, rc_read, err);
    if (!rc_read) rc_read = injected(h, "read");
    if (int rc = agree(h, c, st, rc_read, entry + ": another rank failed during reading (this rank's handle is untouched; free it)")) return rc;
    auto book = [h, t0, tag](const FastqShare &s, uint64_t batches, uint64_t windows) {
        auto &t = h->pipe->times();
        if (s.n_bgzf_slice) t.add((tag + "bgzf_slice_x1").c_str(), (double)s.n_bgzf_slice);
        if (s.n_member_whole) t.add((tag + "member_whole_x1").c_str(), (double)s.n_member_whole);
        if (s.n_text_slice) t.add((tag + "text_slice_x1").c_str(), (double)s.n_text_slice);
        if (s.n_host) t.add((tag + "host_x1").c_str(), (double)s.n_host);
        t.add((tag + "uploaded_bytes").c_str(), (double)s.uploaded_bytes);
        t.add((tag + "batches_x1").c_str(), (double)batches);
        t.add((tag + "windows_x1").c_str(), (double)windows);
        t.add((tag + "read_host_clock").c_str(), now_ms() - t0);
    };
    ShardReads r;
    if (!sh.in_batches) {
        // the share is held: FASTQ — the one pooled batch; FASTA — the files of a pair were packed separately, one batch per file
        book(sh, sh.batches.size(), sh.batches.size());
        for (const FastqShare::Batch &b : sh.batches) r.inst_ub += instances_of(h, b.n_seg, b.n_bases);
        r.n_reads = sh.n_reads;
        r.feed = [&sh](ShardBatchSink &sink) -> int {
            uint64_t reads = 0;
            for (size_t i = 0; i < sh.batches.size(); i++) {
                const FastqShare::Batch &b = sh.batches[i];
                reads += b.n_reads;
                if (int rc = sink.batch(b.n_seg ? b.d_bases() : nullptr, b.n_seg ? b.d_seg_off() : nullptr, b.n_seg, b.n_bases, reads, i + 1, sh.batches.size())) return rc;
            }
            return (int)SHK_OK;
        };
        return shard_preprocess_impl(h, cm, r, n_partitions);
    }
    // several batches: reading and pass 1 take turns (shard_fastq_read_host_clock then holds both)
    r.inst_ub = fasta ? sh.text_ub : sh.text_ub / 2;
    const uint64_t uploaded_before = sh.uploaded_bytes;
    r.feed = [&](ShardBatchSink &sink) -> int {
        FastqShare got;
        std::string e3;
        int rc = read_fastq_share_batches(fq1, n1, fq2, n2, h->k, h->min_qual, s_rank, s_world, h->pipe->device(), st, sink, got, e3, fmt);
        if (rc && !e3.empty()) rc = fail(h, rc, e3);
        got.uploaded_bytes += uploaded_before;
        book(got, got.n_batches, got.n_windows);
        if (!rc) h->n_reads = got.n_reads;
        return rc;
    };
    return shard_preprocess_impl(h, cm, r, n_partitions);
}

// a collective that failed on this rank alone: abort now, so that the peers' waits end (shard_comm.h: comm_stream_wait)
int leave(shk_comm *cm, int rc) {
    if (rc != SHK_OK && cm && cm->c && comm_broken(cm->c)) comm_abort_now(cm->c);
    return rc;
}

}  // namespace

int shard_preprocess_one_impl(shk_handle *h, shk_comm *cm, const void *d_bases, const void *d_seg_off, uint64_t n_seg, uint64_t n_bases,
                              uint64_t n_reads, uint32_t n_partitions) {
    return leave(cm, shard_preprocess_impl(h, cm, one_batch(h, d_bases, d_seg_off, n_seg, n_bases, n_reads), n_partitions));
}
int shard_preprocess_batches_impl(shk_handle *h, shk_comm *cm, uint32_t n_batches, const void *const *d_bases, const void *const *d_seg_off,
                                  const uint64_t *n_seg, const uint64_t *n_bases, uint64_t n_reads, uint32_t n_partitions) {
    return leave(cm, preprocess_batches(h, cm, n_batches, d_bases, d_seg_off, n_seg, n_bases, n_reads, n_partitions));
}
int shard_preprocess_fastq_impl(shk_handle *h, shk_comm *cm, const uint8_t *fq1, size_t n1, const uint8_t *fq2, size_t n2,
                                uint32_t n_partitions, int split, RecFmt fmt) {
    return leave(cm, preprocess_files(h, cm, fq1, n1, fq2, n2, n_partitions, split, fmt));
}
