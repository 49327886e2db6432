// api.cpp — the C ABI of libshk_hip.so (include/shk.h): the stateful AssemblyHelper the
// reference's worker drives (www/src/workers/Assembler.ts:15-39,73-143), its call-order state
// machine, the progress strings (AssemblyPage.vue:458-609) and the JSON getters.
#include <atomic>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <functional>
#include <memory>
#include <mutex>
#include <new>
#include <set>
#include <string>
#include <thread>
#include <vector>

#include "bgzf_write_gpu.h"
#include "deflate_write.h"
#include "end_keys.h"
#include "fasta_gpu.h"
#include "fastq_gpu.h"
#include "inflate_gpu.h"
#include "inflate_mt.h"
#include "preprocess.h"
#include "shard_preprocess.h"
#include "unitig_graph.h"
#include "unitig_graph_gpu.h"

namespace shk { bool spectrum_fit(const uint64_t *histo500, uint32_t *out); }   // fit.cpp

using namespace shk;

static thread_local int g_new_err = 0;
static thread_local std::string g_new_msg;

enum class Poison { Never, AfterFirstBatch, Always };
template <typename F> static int guarded(shk_handle *h, Poison poison, F &&body) {
    if (!h) return SHK_E_PARAM;
    if (h->st == St::Failed) return fail(h, SHK_E_STATE, "the handle failed earlier (" + h->first_err + "): free it and start again");
    DevGuard g(h->pipe ? h->pipe->device() : current_device());
    MemGuard mg(h->mem);
    // device buffers that go out of scope inside the call (early returns included) are parked until the handle's stream
    // has drained, then go back to the pool: nothing in flight can be handed to another handle (device_mem.h)
    DeferScope park(h->pipe);
    int rc;
    try { rc = body(); }
    catch (const std::bad_alloc &) { rc = fail(h, SHK_E_OOM, "out of host memory"); }
    catch (const std::exception &e) { rc = fail(h, SHK_E_INTERNAL, std::string("unexpected exception: ") + e.what()); }
    catch (...) { rc = fail(h, SHK_E_INTERNAL, "unexpected exception"); }
    // a failed call leaves counted batches / a half-built graph behind: a second attempt on the same handle
    // would double-count them, so the handle only accepts shk_free / shk_last_error from here on
    if (rc != SHK_OK && rc != SHK_E_STATE &&
        (poison == Poison::Always || (poison == Poison::AfterFirstBatch && (h->batches_started > 0 || h->st == St::Sharding))))
        { h->st = St::Failed; h->first_err = h->err; }
    return rc;
}

// shk_host_end_key: the writer's end keys in the code the kernels share with the host (end_keys.h)
template <int W> static void host_end_key_t(const char *seq, uint32_t k, int rc, uint32_t o, uint32_t pos, uint64_t *out, uint64_t *entry) {
    const Kmer<W> x = rc ? ek_pack_rc<W>(seq, k) : ek_pack<W>(seq, k);
    for (int j = 0; j < W; j++) out[j] = x.w[j];
    if (entry) *entry = ek_entry(km_hash<W>(x), o, pos);
}

extern "C" {

// the communicators that exist: a handle keeps the one its sharded preprocess ran on, and shk_assemble must find out that it
// has been freed meanwhile (SHK_E_STATE, not a use after free)
static std::mutex g_live_mu;
static std::set<ShardComm *> &live_comms() { static auto *s = new std::set<ShardComm *>(); return *s; }
static bool comm_is_live(ShardComm *c) { std::lock_guard<std::mutex> lk(g_live_mu); return live_comms().count(c) != 0; }

void shk_release_cached_memory(void) { device_pool_trim(); big_trim(); }
// ---- test support: the pool's fill-on-hand-out mode (block_cache.h)
int shk_debug_pool_fill(int on, uint32_t word) { return device_pool_fill(on != 0, word); }
uint64_t shk_debug_pool_filled_bytes(void) { return device_pool_filled_bytes(); }
int shk_debug_pool_probe(size_t bytes, uint32_t *first_word, uint32_t *last_word, size_t *block_bytes) {
    PoolBlock b;
    if (!b.get(bytes)) return SHK_E_OOM;
    std::string err;
    uint32_t first = 0, last = 0;
    if (device_download(&first, b.p, 4, err) || device_download(&last, b.as<char>() + b.bytes - 4, 4, err)) return SHK_E_DEVICE;
    if (first_word) *first_word = first;
    if (last_word) *last_word = last;
    if (block_bytes) *block_bytes = b.bytes;
    return SHK_OK;
}
int shk_measure_stream_read(size_t bytes, int iters, double *gbs) {
    std::string err;
    const int rc = stream_read_gbs(bytes, iters, gbs, err);
    return rc == 0 ? SHK_OK : code_of(Rc::Device, rc);
}

const char *shk_version(void) { return "sparrowhawk_amd 0.1 (gfx950)"; }
int shk_new_error(void) { return g_new_err; }
const char *shk_new_error_message(void) { return g_new_msg.c_str(); }

shk_handle *shk_new(uint32_t k, int verbose, uint32_t min_count, uint32_t min_qual, uint64_t chunk_size,
                    int do_bloom, int do_fit, int no_bubble_collapse, int no_dead_end_removal) {
    g_new_err = 0; g_new_msg.clear();
    if ((k & 1u) == 0 || k < SHK_K_MIN || k > SHK_K_MAX) {
        g_new_err = SHK_E_PARAM; g_new_msg = "k must be odd and within [15, 255]"; return nullptr;
    }
    if (min_qual > 93) { g_new_err = SHK_E_PARAM; g_new_msg = "min_qual out of range"; return nullptr; }
    if (min_count >= SHK_HISTO_BINS) { g_new_err = SHK_E_PARAM; g_new_msg = "min_count out of range"; return nullptr; }
    if (do_bloom && min_count < 3) {     // AssemblyPage.vue:430-432,628-632
        g_new_err = SHK_E_PARAM; g_new_msg = "Bloom mode requires min_count >= 3"; return nullptr;
    }
    shk_handle *h = new (std::nothrow) shk_handle();
    if (!h) { g_new_err = SHK_E_OOM; g_new_msg = "out of host memory"; return nullptr; }
    h->k = k; h->verbose = verbose != 0; h->min_count = min_count; h->min_qual = min_qual;
    h->chunk_size = chunk_size; h->do_bloom = do_bloom != 0; h->do_fit = do_fit != 0;
    h->no_bubble = no_bubble_collapse != 0; h->no_deadend = no_dead_end_removal != 0;
    std::string err;
    {
        MemGuard mg(h->mem);
        h->pipe = make_pipeline((int)k, err);
    }
    if (!h->pipe) { g_new_err = SHK_E_DEVICE; g_new_msg = err; delete h; return nullptr; }
    h->pipe->set_bloom(h->do_bloom);
    h->pipe->set_verbose(h->verbose);
    return h;
}

void shk_free(shk_handle *h) {
    if (!h) return;
    DevGuard g(h->pipe ? h->pipe->device() : current_device());
    delete h->pipe;
    delete h;
}

const char *shk_last_error(shk_handle *h) { return h ? h->err.c_str() : "null handle"; }
void shk_set_progress_cb(shk_handle *h, shk_progress_cb cb, void *user) { if (h) { h->cb = cb; h->cb_user = user; } }

uint32_t shk_shard_record_bytes(shk_handle *h) { return h && h->pipe ? h->pipe->rec_words() * 8u : 0u; }

const char *shk_get_preprocessing_info(shk_handle *h) {
    if (!h) return nullptr;
    if (h->st != St::Preprocessed && h->st != St::Assembled) { h->err = "get_preprocessing_info before preprocess"; return nullptr; }
    return h->pre_json.c_str();
}

static int assemble_impl(shk_handle *h) {
    if (!h) return SHK_E_PARAM;
    if (h->st != St::Preprocessed) return fail(h, SHK_E_STATE, "assemble: preprocess first (and only once)");
    std::string err;
    const double t0 = now_ms();
    h->post("assembly:start");
    if (h->pipe->sharded_graph()) {
        // the graph is spread over the ranks of the communicator shk_shard_preprocess ran on: collective (csrc/shard_graph.h).
        // The three phases run interleaved across ranks; the states are posted in the reference's order.
        if (!h->shard_comm || !comm_is_live(h->shard_comm)) return fail(h, SHK_E_STATE, "assemble: the communicator of the sharded preprocess is gone (shk_comm_free before shk_assemble)");
        h->post("assembly:create_graph");
        std::vector<RawContig> contigs;
        if (h->pipe->n_solid_global() >= (1u << 20)) writer_prewarm(3000);
        const char *dev_json = nullptr; size_t dev_json_len = 0; uint64_t dev_nc = 0;
        int rc = h->pipe->shard_assemble(h->shard_comm, !h->no_deadend, !h->no_bubble, contigs, err, &dev_json, &dev_json_len, &dev_nc);
        // (a failure the other ranks cannot know of has aborted the communicator already: Pipeline::shard_assemble)
        if (rc) return fail_rc(h, Rc::DeviceNoParam, rc, err);
        h->post("assembly:correct_graph");
        h->post("assembly:collapse_graph");
        h->pipe->times().add("assemble_device_total_host_clock", now_ms() - t0);
        h->post("assembly:saving");
        if (dev_json) {                                    // a fragmented assembly: its text was written on the device (csrc/writer_text_gpu.h)
            h->asm_json_dev = dev_json;
            h->pipe->times().add("outputs_host_clock", 0.0);
            h->st = St::Assembled;
            h->post("assembly:end");
            return SHK_OK;
        }
        const double t1 = now_ms();
        build_assembly_text(contigs, h->k, h->text);
        h->asm_json.swap(h->text.json);
        h->pipe->times().add("outputs_host_clock", now_ms() - t1);
        for (auto &kv : h->text.stage_ms) h->pipe->times().add(kv.first, kv.second);
        h->st = St::Assembled;
        h->post("assembly:end");
        return SHK_OK;
    }
    h->post("assembly:create_graph");
    int rc = h->pipe->build_graph(err);
    if (rc) return fail_rc(h, Rc::DeviceNoParam, rc, err);
    h->post("assembly:correct_graph");
    rc = h->pipe->correct(!h->no_deadend, !h->no_bubble, err);
    if (rc) return fail_rc(h, Rc::DeviceNoParam, rc, err);
    h->post("assembly:collapse_graph");
    if (h->pipe->n_solid() >= (1u << 20)) writer_prewarm(3000);     // megabases of output in about a millisecond
    std::vector<RawContig> contigs;
    const char *dev_json = nullptr; size_t dev_json_len = 0; uint64_t dev_nc = 0;
    TextArrival *arrival = nullptr;                    // megabases of contigs: their text is still crossing PCIe when the writer starts
    rc = h->pipe->collapse(contigs, err, &dev_json, &dev_json_len, &dev_nc, &arrival);
    if (rc) return fail_rc(h, Rc::DeviceNoParam, rc, err);
    h->pipe->times().add("assemble_device_total_host_clock", now_ms() - t0);
    h->post("assembly:saving");
    if (dev_json) {                                    // a fragmented assembly: its text was written on the device (csrc/writer_gpu.h)
        h->asm_json_dev = dev_json;
        h->pipe->times().add("outputs_host_clock", 0.0);
        h->st = St::Assembled;
        h->post("assembly:end");
        return SHK_OK;
    }
    const double t1 = now_ms();
    struct ArrivalDone { TextArrival *a; ~ArrivalDone() { if (a) { std::string e; (void)a->finish(e); } } } arrival_done{arrival};   // (also when the writer throws)
    build_assembly_text(contigs, h->k, h->text, arrival);
    if (arrival) { arrival_done.a = nullptr; if (int rc2 = arrival->finish(err)) return fail_rc(h, Rc::DeviceNoParam, rc2, err); }
    h->asm_json.swap(h->text.json);
    h->pipe->times().add("outputs_host_clock", now_ms() - t1);
    if (arrival) h->pipe->times().add("outputs_with_arrival_x1", 1.0);
    for (auto &kv : h->text.stage_ms) h->pipe->times().add(kv.first, kv.second);
    h->st = St::Assembled;
    h->post("assembly:end");
    return SHK_OK;
}

const char *shk_get_assembly(shk_handle *h) {
    if (!h) return nullptr;
    if (h->st != St::Assembled) { h->err = "get_assembly before assemble"; return nullptr; }
    if (h->asm_json_dev) return h->asm_json_dev;
    return h->asm_json.empty() ? "" : (const char *)h->asm_json.data();
}

// ---- the outputs as BGZF files (SPEC S11a; csrc/bgzf_write_gpu.h) --------------------------------------------------------
// The JSON-escaped content of field `key` inside the get_assembly() JSON: from behind `"key":"` to in front of the closing
// quote, the first '"' with an even run of backslashes in front of it.  (The pattern itself cannot stand inside a field: a
// quote of the content is escaped.)
static bool json_string_field(const char *json, size_t len, const char *key, const char *&p, size_t &n) {
    const std::string pat = std::string("\"") + key + "\":\"";
    const char *at = (const char *)memmem(json, len, pat.data(), pat.size());
    if (!at) return false;
    const char *b = at + pat.size(), *end = json + len;
    for (const char *q = b; q < end;) {
        q = (const char *)memchr(q, '"', (size_t)(end - q));
        if (!q) return false;
        size_t run = 0;
        while (q - run > b && q[-1 - (ptrdiff_t)run] == '\\') run++;
        if ((run & 1u) == 0) { p = b; n = (size_t)(q - b); return true; }
        q++;
    }
    return false;
}
static int bgzf_code(int rc) { return rc == -6 ? SHK_E_INTERNAL : code_of(Rc::Device, rc); }

int shk_request_assembly_bgzf(shk_handle *h, uint32_t mask) {
    if (!h) return SHK_E_PARAM;
    if (h->st == St::Assembled || h->st == St::Failed) return fail(h, SHK_E_STATE, "request_assembly_bgzf: call it before assemble");
    if (mask > 15u) return fail(h, SHK_E_PARAM, "request_assembly_bgzf: the mask has bits 0 .. 3 (SHK_OUT_FASTA .. SHK_OUT_GFA2)");
    h->pipe->bgzf_request(mask);
    return SHK_OK;
}

int shk_get_assembly_bgzf(shk_handle *h, int which, const uint8_t **data, size_t *n) {
    return guarded(h, Poison::Never, [&]() -> int {
        if (h->st != St::Assembled) return fail(h, SHK_E_STATE, "get_assembly_bgzf before assemble");
        if (which < SHK_OUT_FASTA || which > SHK_OUT_GFA2 || !data || !n) return fail(h, SHK_E_PARAM, "get_assembly_bgzf: which is SHK_OUT_FASTA, SHK_OUT_DOT, SHK_OUT_GFA1 or SHK_OUT_GFA2");
        if (h->pipe->bgzf_file(which, data, n)) return SHK_OK;
        static const char *const keys[4] = {"outfasta", "outdot", "outgfa", "outgfav2"};
        const char *json = shk_get_assembly(h);
        const size_t len = h->asm_json_dev ? strlen(json) : (h->asm_json.empty() ? 0 : h->asm_json.size() - 1);
        const char *p = nullptr; size_t pn = 0;
        if (!json_string_field(json, len, keys[which], p, pn)) return fail(h, SHK_E_INTERNAL, std::string("get_assembly_bgzf: no field ") + keys[which] + " in the assembly JSON");
        std::string err;
        if (int rc = h->pipe->bgzf_output(which, p, pn, err)) return fail(h, bgzf_code(rc), err);
        if (!h->pipe->bgzf_file(which, data, n)) return fail(h, SHK_E_INTERNAL, "get_assembly_bgzf: the file was not kept");
        return SHK_OK;
    });
}

// the block encoder alone, on the host (csrc/deflate_write.h) and on the current device (csrc/bgzf_write_gpu.hip)
int shk_host_deflate_lengths(const uint32_t counts[257], uint8_t out[257]) {
    if (!counts || !out) return SHK_E_PARAM;
    uint64_t sum = 0;
    for (int i = 0; i < DW_LIT; i++) sum += counts[i];
    if (sum == 0 || sum > 0xFFFFFFFFull) return SHK_E_PARAM;
    DwScratch s;
    dw_rank(counts, DW_LIT, s.order, 0, 1);
    (void)dw_lengths(counts, DW_LIT, 15, s, out);
    return SHK_OK;
}
int shk_host_bgzf_compress(const uint8_t *text, size_t n, uint8_t **out, size_t *out_n) {
    if ((!text && n) || !out || !out_n) return SHK_E_PARAM;
    *out = (uint8_t *)malloc(dw_host_file_bound(n));
    if (!*out) return SHK_E_OOM;
    *out_n = dw_host_file(text, n, *out);
    return SHK_OK;
}
static int device_bgzf_compress(const uint8_t *text, size_t n, bool escaped, uint8_t **out, size_t *out_n, double *ms_kernels) {
    try {
        if ((!text && n) || !out || !out_n) return SHK_E_PARAM;
        *out = nullptr; *out_n = 0;
        std::vector<uint8_t> file; BgzfWriteStats S; std::string err;
        if (int rc = gpu_bgzf_write_host(text, n, escaped, ms_kernels != nullptr, file, S, err)) return bgzf_code(rc);
        *out = (uint8_t *)malloc(file.size());
        if (!*out) return SHK_E_OOM;
        memcpy(*out, file.data(), file.size());
        *out_n = file.size();
        if (ms_kernels) *ms_kernels = S.kernels_ms;
        return SHK_OK;
    } catch (...) { return SHK_E_OOM; }
}
int shk_device_bgzf_compress(const uint8_t *text, size_t n, uint8_t **out, size_t *out_n, double *ms_kernels) {
    return device_bgzf_compress(text, n, false, out, out_n, ms_kernels);
}
int shk_device_bgzf_compress_escaped(const uint8_t *escaped, size_t n, uint8_t **out, size_t *out_n) {
    return device_bgzf_compress(escaped, n, true, out, out_n, nullptr);
}

// ---- packer ------------------------------------------------------------------------------
static int packed_to_caller(PackedReads &pr, shk_packed *out);      // a finished copy in malloc'ed memory (shk_packed_free)
int shk_pack_fastq(const uint8_t *fq, size_t n, uint32_t k, uint32_t min_qual, shk_packed *out, const char **errp) {
    static thread_local std::string msg;
    if (!out) return SHK_E_PARAM;
    PackedReads pr;
    int rc = pack_fastq(fq, n, k, min_qual, pr, msg);
    if (rc) { if (errp) *errp = msg.c_str(); return code_of(Rc::Parser, rc); }
    return packed_to_caller(pr, out);
}
int shk_pack_fasta(const uint8_t *fa, size_t n, uint32_t k, shk_packed *out, const char **errp) {
    static thread_local std::string msg;
    if (!out || (!fa && n)) return SHK_E_PARAM;
    if ((k & 1u) == 0 || k < SHK_K_MIN || k > SHK_K_MAX) { msg = "k must be odd and within [15, 255]"; if (errp) *errp = msg.c_str(); return SHK_E_PARAM; }
    try {
        PackedReads pr;
        int rc = pack_fasta(fa, n, k, pr, msg);
        if (rc) { if (errp) *errp = msg.c_str(); return code_of(Rc::Parser, rc); }
        return packed_to_caller(pr, out);
    } catch (...) { return SHK_E_OOM; }
}
// the device FASTA packer alone (tests): the batch comes back to the host (shk_packed_free); *route: "device", "host" (the
// device packer declined and the host packer took the text), or the message of a failure
int shk_device_pack_fasta(const uint8_t *fa1, size_t n1, const uint8_t *fa2, size_t n2, uint32_t k, shk_packed *out, const char **route) {
    static thread_local std::string msg;
    try {
        if (!out || (!fa1 && n1) || (!fa2 && n2)) return SHK_E_PARAM;
        *out = shk_packed();
        if (route) *route = "";
        if ((k & 1u) == 0 || k < SHK_K_MIN || k > SHK_K_MAX) { msg = "k must be odd and within [15, 255]"; if (route) *route = msg.c_str(); return SHK_E_PARAM; }
        ByteVec st1, st2; const uint8_t *t1 = nullptr, *t2 = nullptr; size_t l1 = 0, l2 = 0;
        if (int ri = maybe_inflate_pair(fa1, n1, fa2, n2, st1, st2, t1, l1, t2, l2, msg)) { if (route) *route = msg.c_str(); return code_of(Rc::Inflater, ri); }
        GpuPacked gp;
        struct Free { GpuPacked &g; ~Free() { gpu_packed_free(g); } } free_gp{gp};
        const int rc = gpu_pack_fasta(t1, l1, fa2 ? t2 : nullptr, l2, k, 0, nullptr, gp, msg);
        if (rc < 0) { if (route) *route = msg.c_str(); return code_of(Rc::Device, rc); }
        if (rc == 1) {
            PackedReads pr;
            int rh = pack_fasta(t1, l1, k, pr, msg);
            if (!rh && fa2) rh = pack_fasta(t2, l2, k, pr, msg);
            if (rh) msg = "host: " + msg;                  // (the route, then the host packer's message)
            if (route) *route = rh ? msg.c_str() : "host";
            return rh ? code_of(Rc::Parser, rh) : packed_to_caller(pr, out);
        }
        const size_t nw = (size_t)(gp.n_bases >> 4) + 2;
        out->bases = (uint32_t *)calloc(nw, 4);
        out->seg_off = (uint32_t *)calloc((size_t)gp.n_seg + 1, 4);
        if (!out->bases || !out->seg_off) { shk_packed_free(out); return SHK_E_OOM; }
        if (device_download(out->bases, gp.d_bases, nw * 4, msg) || device_download(out->seg_off, gp.d_seg_off, ((size_t)gp.n_seg + 1) * 4, msg)) {
            shk_packed_free(out);
            if (route) *route = msg.c_str();
            return SHK_E_DEVICE;
        }
        out->n_seg = gp.n_seg; out->n_bases = gp.n_bases; out->n_reads = gp.n_reads; out->n_input_bases = gp.n_input_bases;
        if (route) *route = "device";
        return SHK_OK;
    } catch (...) { return SHK_E_OOM; }
}
static int packed_to_caller(PackedReads &pr, shk_packed *out) {
    pr.finish();
    out->n_seg = pr.n_seg(); out->n_bases = pr.n_bases; out->n_reads = pr.n_reads; out->n_input_bases = pr.n_input_bases;
    out->bases = (uint32_t *)malloc(pr.bases.size() * 4);
    out->seg_off = (uint32_t *)malloc(pr.seg_off.size() * 4);
    if (!out->bases || !out->seg_off) { free(out->bases); free(out->seg_off); return SHK_E_OOM; }
    memcpy(out->bases, pr.bases.data(), pr.bases.size() * 4);
    memcpy(out->seg_off, pr.seg_off.data(), pr.seg_off.size() * 4);
    return SHK_OK;
}
void shk_packed_free(shk_packed *p) { if (p) { free(p->bases); free(p->seg_off); p->bases = nullptr; p->seg_off = nullptr; } }

// ---- stage inspection -----------------------------------------------------------------------
uint32_t shk_key_words(shk_handle *h) { return h ? (2 * h->k + 63) / 64 : 0; }
uint64_t shk_total_instances(shk_handle *h) { return h && h->pipe ? h->pipe->total_instances() : 0; }
uint64_t shk_n_distinct(shk_handle *h) { return h && h->pipe ? h->pipe->n_distinct() : 0; }
uint64_t shk_n_solid(shk_handle *h) { return h && h->pipe ? h->pipe->n_solid() : 0; }
uint32_t shk_used_min_count(shk_handle *h) { return h ? h->used_min_count : 0; }

static int get_distinct_impl(shk_handle *h, uint64_t *keys, uint32_t *counts, uint64_t cap) {
    if (!h) return SHK_E_PARAM;
    if (h->st != St::Preprocessed) return fail(h, SHK_E_STATE, "get_distinct: only between preprocess and assemble");
    std::string err; int rc = h->pipe->get_distinct(keys, counts, cap, err);
    return rc ? fail(h, rc == -1 ? SHK_E_PARAM : SHK_E_DEVICE, err) : SHK_OK;
}
static int get_solid_impl(shk_handle *h, uint64_t *keys, uint32_t *counts, uint64_t cap) {
    if (!h) return SHK_E_PARAM;
    if (h->st != St::Preprocessed && h->st != St::Assembled) return fail(h, SHK_E_STATE, "get_solid before preprocess");
    std::string err; int rc = h->pipe->get_solid(keys, counts, cap, err);
    return rc ? fail(h, rc == -1 ? SHK_E_PARAM : SHK_E_DEVICE, err) : SHK_OK;
}
int shk_get_histo(shk_handle *h, uint64_t *histo500) {
    if (!h) return SHK_E_PARAM;
    if (h->st != St::Preprocessed && h->st != St::Assembled) return fail(h, SHK_E_STATE, "get_histo before preprocess");
    memcpy(histo500, h->histo, sizeof h->histo);
    return SHK_OK;
}
static int get_adjacency_impl(shk_handle *h, uint8_t *adj_initial, uint8_t *adj_final, uint8_t *alive, uint64_t cap) {
    if (!h) return SHK_E_PARAM;
    if (h->st != St::Assembled) return fail(h, SHK_E_STATE, "get_adjacency before assemble");
    std::string err; int rc = h->pipe->get_adjacency(adj_initial, adj_final, alive, cap, err);
    return rc ? fail(h, rc == -1 ? SHK_E_PARAM : SHK_E_DEVICE, err) : SHK_OK;
}
const char *shk_get_timings(shk_handle *h) {
    if (!h || !h->pipe) return "{}";
    DevGuard g(h->pipe->device());
    std::string j = "{";
    bool first = true;
    for (auto &kv : h->pipe->times().ms) {
        if (!first) j += ",";
        first = false;
        char buf[64]; snprintf(buf, sizeof buf, "%.6f", kv.second);
        j += "\"" + kv.first + "\":" + buf;
    }
    {   // not a time: the most device memory this handle held at once, in bytes (Assembler.ts:69-71,137 reports peak memory)
        char buf[96]; snprintf(buf, sizeof buf, "%s\"peak_device_bytes\":%llu,\"device_bytes_now\":%llu", first ? "" : ",",
                               (unsigned long long)mem_acct_peak(h->mem), (unsigned long long)mem_acct_current(h->mem));
        j += buf;
    }
    j += "}";
    h->timings_json.swap(j);
    return h->timings_json.c_str();
}

uint64_t shk_peak_device_bytes(shk_handle *h) { return h ? mem_acct_peak(h->mem) : 0; }
void shk_host_mem_counter(const int64_t *deltas, size_t n, uint64_t *peak, uint64_t *current) { mem_acct_replay(deltas, n, peak, current); }

// ---- collectives inside the library (shard_comm.hip: RCCL) ---------------------------------------------
static thread_local std::string g_comm_err;

int shk_comm_unique_id(uint8_t id[SHK_UNIQUE_ID_BYTES]) {
    try { return comm_unique_id(id, g_comm_err) == 0 ? SHK_OK : SHK_E_DEVICE; }
    catch (...) { g_comm_err = "unexpected exception"; return SHK_E_INTERNAL; }
}
shk_comm *shk_comm_init(const uint8_t id[SHK_UNIQUE_ID_BYTES], int rank, int world) {
    try {
        if (!id) { g_comm_err = "null id"; return nullptr; }
        ShardComm *c = comm_create(id, rank, world, g_comm_err);
        if (!c) return nullptr;
        shk_comm *w = new (std::nothrow) shk_comm();
        if (!w) { comm_destroy(c); g_comm_err = "out of host memory"; return nullptr; }
        w->c = c;
        { std::lock_guard<std::mutex> lk(g_live_mu); live_comms().insert(c); }
        return w;
    } catch (...) { g_comm_err = "unexpected exception"; return nullptr; }
}
const char *shk_comm_error(void) { return g_comm_err.c_str(); }
int shk_comm_rank(const shk_comm *c) { return c ? comm_rank(c->c) : 0; }
int shk_comm_world(const shk_comm *c) { return c ? comm_world(c->c) : 0; }
void shk_comm_free(shk_comm *c) {
    if (!c) return;
    DevGuard g(comm_device(c->c));
    { std::lock_guard<std::mutex> lk(g_live_mu); live_comms().erase(c->c); }
    comm_destroy(c->c);
    delete c;
}
// (the collective calls abort a communicator whose collective failed on this rank alone before they return: shard_preprocess.cpp)
int shk_shard_preprocess(shk_handle *h, shk_comm *c, const void *d_bases, const void *d_seg_off, uint64_t n_seg,
                         uint64_t n_bases, uint64_t n_reads, uint32_t n_partitions) {
    return guarded(h, Poison::AfterFirstBatch, [&] { return shard_preprocess_one_impl(h, c, d_bases, d_seg_off, n_seg, n_bases, n_reads, n_partitions); });
}
int shk_shard_preprocess_batches(shk_handle *h, shk_comm *c, uint32_t n_batches, const void *const *d_bases, const void *const *d_seg_off,
                                 const uint64_t *n_seg, const uint64_t *n_bases, uint64_t n_reads, uint32_t n_partitions) {
    return guarded(h, Poison::AfterFirstBatch, [&] { return shard_preprocess_batches_impl(h, c, n_batches, d_bases, d_seg_off, n_seg, n_bases, n_reads, n_partitions); });
}
int shk_shard_preprocess_fastq(shk_handle *h, shk_comm *c, const uint8_t *fq1, size_t n1, const uint8_t *fq2, size_t n2,
                               uint32_t n_partitions, int split) {
    return guarded(h, Poison::AfterFirstBatch, [&] { return shard_preprocess_fastq_impl(h, c, fq1, n1, fq2, n2, n_partitions, split, RecFmt::Fastq); });
}
int shk_shard_preprocess_fasta(shk_handle *h, shk_comm *c, const uint8_t *fa1, size_t n1, const uint8_t *fa2, size_t n2,
                               uint32_t n_partitions, int split) {
    return guarded(h, Poison::AfterFirstBatch, [&] { return shard_preprocess_fastq_impl(h, c, fa1, n1, fa2, n2, n_partitions, split, RecFmt::Fasta); });
}
int shk_plan_exchange(const uint64_t *part_records_all, uint32_t world, uint32_t n_partitions, uint32_t rank,
                      uint64_t *base, uint64_t *send_counts, uint64_t *recv_counts, uint64_t *run_off, uint32_t *run_cnt) {
    try {
        ExchangePlan pl; std::string err;
        if (!base || !send_counts || !recv_counts || !run_off || !run_cnt) return SHK_E_PARAM;
        if (plan_exchange(part_records_all, world, n_partitions, rank, pl, err)) return SHK_E_PARAM;
        memcpy(base, pl.base.data(), pl.base.size() * 8);
        memcpy(send_counts, pl.send_counts.data(), (size_t)world * 8);
        memcpy(recv_counts, pl.recv_counts.data(), (size_t)world * 8);
        memcpy(run_off, pl.run_off.data(), pl.run_off.size() * 8);
        memcpy(run_cnt, pl.run_cnt.data(), pl.run_cnt.size() * 4);
        return SHK_OK;
    } catch (...) { return SHK_E_OOM; }
}
int64_t shk_plan_bgzf_windows(const uint32_t *isize, uint64_t n_blocks, uint64_t budget, uint64_t *first_block, uint64_t cap) {
    try {
        if ((!isize && n_blocks) || (!first_block && cap)) return SHK_E_PARAM;
        std::vector<uint64_t> first;
        if (plan_bgzf_windows(isize, (size_t)n_blocks, budget, first)) return SHK_E_PARAM;
        for (size_t i = 0; i < first.size() && i < cap; i++) first_block[i] = first[i];
        return (int64_t)first.size();
    } catch (...) { return SHK_E_OOM; }
}
int64_t shk_plan_share_windows(const uint32_t *isize, uint64_t n_blocks, uint32_t world, uint32_t rank, uint64_t budget, uint64_t *first_block,
                               uint64_t cap) {
    try {
        if ((!isize && n_blocks) || (!first_block && cap) || !world || rank >= world) return SHK_E_PARAM;
        for (uint64_t i = 0; i < n_blocks; i++) if (isize[i] > 65536) return SHK_E_PARAM;
        std::vector<uint64_t> first; uint64_t run_end = 0;
        if (plan_share_windows(isize, (size_t)n_blocks, world, rank, budget, first, run_end)) return SHK_E_PARAM;
        for (size_t i = 0; i < first.size() && i < cap; i++) first_block[i] = first[i];
        return (int64_t)first.size();
    } catch (...) { return SHK_E_OOM; }
}
uint64_t shk_host_last_record_start(const uint8_t *text, size_t n) { return (text || !n) ? last_record_start(text, n) : UINT64_MAX; }
int shk_device_last_record_start(const uint8_t *text, size_t n, uint64_t *at) {
    try {
        if ((!text && n) || !at) return SHK_E_PARAM;
        std::string err;
        const int rc = gpu_last_record_start(text, n, current_device(), *at, err);
        return rc ? code_of(Rc::DeviceNoParam, rc) : SHK_OK;
    } catch (...) { return SHK_E_OOM; }
}
uint64_t shk_host_first_record_start(const uint8_t *text, size_t n, uint64_t from) { return (text || !n) ? first_record_start(text, n, (size_t)std::min<uint64_t>(from, n)) : UINT64_MAX; }
int shk_device_first_record_start(const uint8_t *text, size_t n, uint64_t from, uint64_t *at) {
    try {
        if ((!text && n) || !at) return SHK_E_PARAM;
        std::string err;
        const int rc = gpu_first_record_start(text, n, from, current_device(), *at, err);
        return rc ? code_of(Rc::DeviceNoParam, rc) : SHK_OK;
    } catch (...) { return SHK_E_OOM; }
}
uint64_t shk_host_first_fasta_record_start(const uint8_t *text, size_t n, uint64_t from) {
    return (text || !n) ? fasta_first_record_start(text, n, (size_t)std::min<uint64_t>(from, n)) : UINT64_MAX;
}
uint64_t shk_host_last_fasta_record_start(const uint8_t *text, size_t n) { return (text || !n) ? fasta_last_record_start(text, n) : UINT64_MAX; }
int shk_device_first_fasta_record_start(const uint8_t *text, size_t n, uint64_t from, uint64_t *at) {
    try {
        if ((!text && n) || !at) return SHK_E_PARAM;
        std::string err;
        const int rc = gpu_fasta_record_start(text, n, false, from, current_device(), *at, err);
        return rc ? code_of(Rc::DeviceNoParam, rc) : SHK_OK;
    } catch (...) { return SHK_E_OOM; }
}
int shk_device_last_fasta_record_start(const uint8_t *text, size_t n, uint64_t *at) {
    try {
        if ((!text && n) || !at) return SHK_E_PARAM;
        std::string err;
        const int rc = gpu_fasta_record_start(text, n, true, 0, current_device(), *at, err);
        return rc ? code_of(Rc::DeviceNoParam, rc) : SHK_OK;
    } catch (...) { return SHK_E_OOM; }
}
int64_t shk_plan_fastq_slices(const uint32_t *isize, uint64_t n_blocks, uint32_t world, uint64_t *first_block) {
    try {
        if ((!isize && n_blocks) || !first_block || !world) return SHK_E_PARAM;
        for (uint64_t i = 0; i < n_blocks; i++) if (isize[i] > 65536) return SHK_E_PARAM;
        std::vector<uint64_t> first;
        plan_fastq_slices(isize, (size_t)n_blocks, world, first);
        memcpy(first_block, first.data(), first.size() * 8);
        return (int64_t)world;
    } catch (...) { return SHK_E_OOM; }
}
// the routes of shk_shard_preprocess_fastq / _fasta with split = 1, without a communicator: the packed batch of slice `rank` of
// `world` comes back to the host (shk_packed_free).  FASTA: the files of a pair are packed separately, their batches come
// back as one (file 1's segments, then file 2's).
static int device_pack_slice(RecFmt fmt, const uint8_t *f1, size_t n1, const uint8_t *f2, size_t n2, uint32_t k, uint32_t min_qual,
                             uint32_t rank, uint32_t world, shk_packed *out, uint64_t *uploaded_bytes, const char **route) {
    static thread_local std::string msg, route_s;
    try {
        if (!out) return SHK_E_PARAM;
        *out = shk_packed();
        if (route) *route = "";
        if ((k & 1u) == 0 || k < SHK_K_MIN || k > SHK_K_MAX) { msg = "k must be odd and within [15, 255]"; if (route) *route = msg.c_str(); return SHK_E_PARAM; }
        FastqShare sh;
        const int rc = read_fastq_share(f1, n1, f2, n2, k, min_qual, rank, world, current_device(), nullptr, sh, msg, false, fmt);
        if (uploaded_bytes) *uploaded_bytes = sh.uploaded_bytes;
        if (rc) { if (route) *route = msg.c_str(); return rc; }      // (on failure *route carries the message)
        const size_t nw = (size_t)(sh.n_bases >> 4) + 2;
        out->bases = (uint32_t *)calloc(nw, 4);
        out->seg_off = (uint32_t *)calloc((size_t)sh.n_seg + 1, 4);
        if (!out->bases || !out->seg_off) { shk_packed_free(out); return SHK_E_OOM; }
        uint64_t base_at = 0, seg_at = 0;
        for (const FastqShare::Batch &b : sh.batches) {
            if (!b.n_seg) continue;
            int bad;
            if (sh.batches.size() == 1) bad = device_download(out->bases, b.d_bases(), nw * 4, msg) || device_download(out->seg_off, b.d_seg_off(), ((size_t)b.n_seg + 1) * 4, msg);
            else {
                std::vector<uint32_t> bases((size_t)(b.n_bases >> 4) + 2), seg((size_t)b.n_seg + 1);
                bad = device_download(bases.data(), b.d_bases(), bases.size() * 4, msg) || device_download(seg.data(), b.d_seg_off(), seg.size() * 4, msg);
                for (uint64_t i = 0; !bad && i < b.n_bases; i++) {   // (a test entry: base by base behind what file 1 gave)
                    const uint32_t code = (bases[(size_t)(i >> 4)] >> (2 * (i & 15))) & 3u;
                    out->bases[(size_t)((base_at + i) >> 4)] |= code << (2 * ((base_at + i) & 15));
                }
                for (uint64_t j = 1; !bad && j <= b.n_seg; j++) out->seg_off[(size_t)(seg_at + j)] = (uint32_t)(base_at + seg[(size_t)j]);
                base_at += b.n_bases; seg_at += b.n_seg;
            }
            if (bad) {
                shk_packed_free(out);
                if (route) *route = msg.c_str();
                return SHK_E_DEVICE;
            }
        }
        out->n_seg = sh.n_seg; out->n_bases = sh.n_bases; out->n_reads = sh.n_reads; out->n_input_bases = sh.n_input_bases;
        route_s = sh.route;
        if (route) *route = route_s.c_str();
        return SHK_OK;
    } catch (...) { return SHK_E_OOM; }
}
int shk_device_pack_fastq_slice(const uint8_t *fq1, size_t n1, const uint8_t *fq2, size_t n2, uint32_t k, uint32_t min_qual,
                                uint32_t rank, uint32_t world, shk_packed *out, uint64_t *uploaded_bytes, const char **route) {
    return device_pack_slice(RecFmt::Fastq, fq1, n1, fq2, n2, k, min_qual, rank, world, out, uploaded_bytes, route);
}
int shk_device_pack_fasta_slice(const uint8_t *fa1, size_t n1, const uint8_t *fa2, size_t n2, uint32_t k, uint32_t rank, uint32_t world,
                                shk_packed *out, uint64_t *uploaded_bytes, const char **route) {
    return device_pack_slice(RecFmt::Fasta, fa1, n1, fa2, n2, k, 0, rank, world, out, uploaded_bytes, route);
}
uint32_t shk_choose_partitions(uint64_t total_instances_ub, uint32_t world, uint32_t key_words) {
    return choose_partitions(total_instances_ub, world ? world : 1, key_words <= 1 ? 100000 : 40000);
}

// ---- the guarded entry points (device guard, no exception across the ABI, failed-handle state) ----
int shk_preprocess(shk_handle *h, const uint8_t *fq1, size_t n1, const uint8_t *fq2, size_t n2) {
    return guarded(h, Poison::AfterFirstBatch, [&] { return preprocess_impl(h, fq1, n1, fq2, n2); });
}
int shk_preprocess_fasta(shk_handle *h, const uint8_t *fa1, size_t n1, const uint8_t *fa2, size_t n2) {
    return guarded(h, Poison::AfterFirstBatch, [&] { return preprocess_fasta_impl(h, fa1, n1, fa2, n2); });
}
int shk_push_reads(shk_handle *h, const uint8_t *chunk, size_t n) {
    return guarded(h, Poison::AfterFirstBatch, [&] { return push_reads_impl(h, chunk, n); });
}
int shk_finish_reads(shk_handle *h) {
    return guarded(h, Poison::AfterFirstBatch, [&] { return finish_reads_impl(h); });
}
int shk_preprocess_packed_device(shk_handle *h, const void *d_bases, const void *d_seg_off, uint64_t n_seg,
                                 uint64_t n_bases, uint64_t n_reads) {
    return guarded(h, Poison::AfterFirstBatch, [&] { return preprocess_packed_device_impl(h, d_bases, d_seg_off, n_seg, n_bases, n_reads); });
}
int shk_preprocess_packed_host(shk_handle *h, const uint32_t *bases, const uint32_t *seg_off, uint64_t n_seg, uint64_t n_bases,
                               uint64_t n_reads) {
    return guarded(h, Poison::AfterFirstBatch, [&] { return preprocess_packed_host_impl(h, bases, seg_off, n_seg, n_bases, n_reads); });
}
int shk_shard_partition(shk_handle *h, const void *d_bases, const void *d_seg_off, uint64_t n_seg, uint64_t n_bases,
                        uint64_t n_reads, uint32_t n_partitions, uint64_t *part_records) {
    return guarded(h, Poison::AfterFirstBatch, [&] { return shard_partition_impl(h, d_bases, d_seg_off, n_seg, n_bases, n_reads, n_partitions, part_records); });
}
int shk_shard_pack(shk_handle *h, void *d_send, const uint64_t *base_records, uint32_t n_partitions) {
    return guarded(h, Poison::AfterFirstBatch, [&] { return shard_pack_impl(h, d_send, base_records, n_partitions); });
}
int shk_shard_count(shk_handle *h, const void *d_recv, const uint64_t *run_off, const uint32_t *run_cnt,
                    uint32_t n_owned, uint32_t n_sources, uint64_t *histo500_local, uint64_t *n_instances_local) {
    return guarded(h, Poison::AfterFirstBatch, [&] { return shard_count_impl(h, d_recv, run_off, run_cnt, n_owned, n_sources, histo500_local, n_instances_local); });
}
int shk_shard_rows(shk_handle *h, const uint64_t *histo500_global, const void **d_keys, const void **d_cnt,
                   uint64_t *n_rows, uint32_t *used_min_count) {
    return guarded(h, Poison::AfterFirstBatch, [&] { return shard_rows_impl(h, histo500_global, d_keys, d_cnt, n_rows, used_min_count); });
}
int shk_shard_set_solid(shk_handle *h, const void *const *d_keys, const void *d_cnt, uint64_t n_rows,
                        uint64_t n_instances_global) {
    return guarded(h, Poison::AfterFirstBatch, [&] { return shard_set_solid_impl(h, d_keys, d_cnt, n_rows, n_instances_global); });
}
int shk_assemble(shk_handle *h) {
    return guarded(h, Poison::Always, [&] { return assemble_impl(h); });
}
int shk_get_distinct(shk_handle *h, uint64_t *keys, uint32_t *counts, uint64_t cap) {
    return guarded(h, Poison::Never, [&] { return get_distinct_impl(h, keys, counts, cap); });
}
int shk_get_solid(shk_handle *h, uint64_t *keys, uint32_t *counts, uint64_t cap) {
    return guarded(h, Poison::Never, [&] { return get_solid_impl(h, keys, counts, cap); });
}
int shk_get_adjacency(shk_handle *h, uint8_t *adj_initial, uint8_t *adj_final, uint8_t *alive, uint64_t cap) {
    return guarded(h, Poison::Never, [&] { return get_adjacency_impl(h, adj_initial, adj_final, alive, cap); });
}

// ---- host-only self tests --------------------------------------------------------------------
int shk_host_canonical(const char *seq, uint32_t k, uint64_t *out_words, int *orient) {
    if (!seq || !out_words || (k & 1u) == 0 || k > SHK_K_MAX) return SHK_E_PARAM;
    return host_canonical(seq, k, out_words, orient) == 0 ? SHK_OK : SHK_E_PARAM;
}
uint64_t shk_host_nthash(const char *seq, uint32_t k) { return host_nthash(seq, k); }
int shk_host_end_key(const char *seq, uint32_t k, int rc, uint32_t orientation, uint32_t pos, uint64_t *out_words, uint64_t *entry) {
    if (!seq || !out_words || k < 1 || k > SHK_K_MAX || orientation > 1 || pos > 0x7FFFFFFFu) return SHK_E_PARAM;
    switch ((2 * k + 63) / 64) {
        case 1: host_end_key_t<1>(seq, k, rc, orientation, pos, out_words, entry); break;
        case 2: host_end_key_t<2>(seq, k, rc, orientation, pos, out_words, entry); break;
        case 3: host_end_key_t<3>(seq, k, rc, orientation, pos, out_words, entry); break;
        case 4: host_end_key_t<4>(seq, k, rc, orientation, pos, out_words, entry); break;
        case 5: host_end_key_t<5>(seq, k, rc, orientation, pos, out_words, entry); break;
        case 6: host_end_key_t<6>(seq, k, rc, orientation, pos, out_words, entry); break;
        case 7: host_end_key_t<7>(seq, k, rc, orientation, pos, out_words, entry); break;
        case 8: host_end_key_t<8>(seq, k, rc, orientation, pos, out_words, entry); break;
        default: return SHK_E_PARAM;
    }
    return SHK_OK;
}
int shk_host_fit(const uint64_t *histo500, uint32_t *used) { return spectrum_fit(histo500, used) ? 1 : 0; }
char *shk_host_assembly_json(const char *seqs, const uint64_t *offsets, const uint64_t *kc, uint64_t n_contigs, uint32_t k) {
    try {
        if ((!seqs && n_contigs) || !offsets || (!kc && n_contigs)) return nullptr;
        std::vector<RawContig> contigs((size_t)n_contigs);
        for (uint64_t i = 0; i < n_contigs; i++) {
            if (offsets[i + 1] < offsets[i] + k) return nullptr;            // a unitig spells at least one k-mer
            contigs[i].ext = seqs + offsets[i]; contigs[i].ext_n = (size_t)(offsets[i + 1] - offsets[i]); contigs[i].kc = kc[i];
        }
        AssemblyText text;
        build_assembly_text(contigs, k, text);
        char *out = (char *)malloc(text.json.size());        // (the JSON carries its terminator)
        if (!out) return nullptr;
        memcpy(out, text.json.data(), text.json.size());
        return out;
    } catch (...) { return nullptr; }
}
// the same writer on text that ARRIVES while it works (the device path hands it text that is still crossing PCIe): a thread
// releases the bytes piece by piece into a buffer that starts out as garbage, the contigs carry their ends as the device
// path's do — the JSON must be the one shk_host_assembly_json gives (tests; no GPU)
char *shk_host_assembly_json_arriving(const char *seqs, const uint64_t *offsets, const uint64_t *kc, uint64_t n_contigs, uint32_t k,
                                      uint64_t piece_bytes, uint32_t delay_us) {
    try {
        if ((!seqs && n_contigs) || !offsets || (!kc && n_contigs) || !piece_bytes) return nullptr;
        const size_t total = (size_t)offsets[n_contigs];
        struct Fake : TextArrival {
            std::vector<char> buf; std::atomic<size_t> ready{0};
            const char *base() const override { return buf.data(); }
            size_t total() const override { return buf.size(); }
            void wait_range(size_t, size_t end) override { if (end > buf.size()) end = buf.size(); while (ready.load(std::memory_order_acquire) < end) std::this_thread::yield(); }
            int finish(std::string &) override { wait_all(); return 0; }
        } fake;
        fake.buf.assign(total, '#');                       // (what has not arrived is not sequence)
        const uint32_t E = std::max<uint32_t>(k, 32);
        std::vector<char> ends((size_t)n_contigs * 2 * E, 0);
        std::vector<RawContig> contigs((size_t)n_contigs);
        for (uint64_t i = 0; i < n_contigs; i++) {
            if (offsets[i + 1] < offsets[i] + k) return nullptr;
            const size_t len = (size_t)(offsets[i + 1] - offsets[i]), m = std::min<size_t>(E, len);
            contigs[i].ext = fake.buf.data() + offsets[i]; contigs[i].ext_n = len; contigs[i].kc = kc[i];
            memcpy(&ends[(size_t)i * 2 * E], seqs + offsets[i], m);
            memcpy(&ends[(size_t)i * 2 * E + E], seqs + offsets[i] + len - m, m);
            contigs[i].head = &ends[(size_t)i * 2 * E]; contigs[i].tail = contigs[i].head + E; contigs[i].ends_n = (uint32_t)m;
        }
        std::thread feeder([&] {
            for (size_t o = 0; o < total; o += (size_t)piece_bytes) {
                if (delay_us) std::this_thread::sleep_for(std::chrono::microseconds(delay_us));
                const size_t m = std::min<size_t>((size_t)piece_bytes, total - o);
                memcpy(fake.buf.data() + o, seqs + o, m);
                fake.ready.store(o + m, std::memory_order_release);
            }
        });
        struct Join { std::thread &t; ~Join() { if (t.joinable()) t.join(); } } join{feeder};
        AssemblyText text;
        build_assembly_text(contigs, k, text, total ? &fake : nullptr);
        char *out = (char *)malloc(text.json.size());
        if (!out) return nullptr;
        memcpy(out, text.json.data(), text.json.size());
        return out;
    } catch (...) { return nullptr; }
}
// the device twin of shk_host_assembly_json (csrc/writer_text_gpu.h): the same parameters, the same bytes; on the current device
char *shk_device_assembly_json(const char *seqs, const uint64_t *offsets, const uint64_t *kc, uint64_t n_contigs, uint32_t k, const char **why) {
    static thread_local std::string msg;
    auto say = [&](const std::string &m) { if (why) { msg = m; *why = msg.c_str(); } };
    try {
        say("");
        if ((!seqs && n_contigs) || !offsets || (!kc && n_contigs) || k < 1 || k > SHK_K_MAX) { say("bad parameters"); return nullptr; }
        for (uint64_t i = 0; i < n_contigs; i++)
            if (offsets[i + 1] < offsets[i] + k) { say("offsets not ascending, or a contig shorter than k"); return nullptr; }      // (the host twin's refusal)
        if (n_contigs == 0) return shk_host_assembly_json(seqs, offsets, kc, 0, k);      // (no contig: the literals alone)
        std::string err;
        std::unique_ptr<IPipeline> pipe(make_pipeline((int)k, err));
        if (!pipe) { say(err); return nullptr; }
        const char *json = nullptr, *wn = ""; size_t len = 0;
        char *out = nullptr;
        {
            DeferScope park(pipe.get());                   // (the writer's device buffers go back once its stream is idle)
            const int rc = pipe->text_assembly_json(seqs, offsets, kc, n_contigs, &json, &len, &wn, err);
            if (rc == 1) { say(wn); return nullptr; }
            if (rc || !json) { say(err); return nullptr; }
            out = (char *)malloc(len + 1);
            if (!out) { say("out of host memory"); return nullptr; }
            memcpy(out, json, len + 1);                    // (the JSON carries its terminator)
        }
        return out;
    } catch (...) { say("out of host memory"); return nullptr; }
}
void shk_host_free(void *p) { free(p); }
// the device inflater alone (csrc/inflate_gpu.hip): 0 = *out (malloc'd, shk_host_free) holds the bytes of the member or of
// the BGZF file; 1 = the file was not taken (*why says why: the product then reads it on the host); < 0 = error
int shk_device_gunzip(const uint8_t *gz, size_t n, uint8_t **out, size_t *out_n, const char **why, double *ms_total) {
    try {
        if (!gz || !out || !out_n) return SHK_E_PARAM;
        *out = nullptr; *out_n = 0;
        static thread_local std::string msg;
        std::string err;
        // a BGZF file through the windows of shk_preprocess's route 2: where SHK_GUNZIP_DEVICE_WINDOW is set, or the text
        // reaches 4 GiB.  Every window is cut at its last record start and its rest carried into the next, as the route does
        // (text without one, or a carry beyond the room for it: the window is handed on whole); the bytes are all returned.
        {
            const BgzfWindowKnob window = bgzf_window_knob(UINT64_MAX);      // (no batch here to fit a window into)
            size_t bs = 0;
            BgzfChain chain; const char *why_not = "";
            if (n >= 18 && bgzf_block(gz, n, bs) && bgzf_walk(gz, n, chain, why_not) == 0 && chain.text && (window.set || chain.text >= (1ull << 32))) {
                auto say = [&](const std::string &m) { if (why) { msg = m; *why = msg.c_str(); } };
                if (bgzf_cut_windows(chain, window.bytes)) return SHK_E_INTERNAL;
                const double t0 = now_ms();
                uint8_t *o = (uint8_t *)malloc((size_t)chain.text);
                if (!o) return SHK_E_OOM;
                struct Free { uint8_t *&p; ~Free() { free(p); } } guard{o};
                BgzfWindows bw;
                int rc = bw.open(gz, &chain, current_device(), nullptr, err);
                if (rc == 1) { say("out of device memory"); return 1; }
                if (rc) { say(err); return code_of(Rc::DeviceNoParam, rc); }
                uint64_t carry = 0, done = 0;
                for (size_t w = 0; w < chain.windows.size(); w++) {
                    const char *wn = "";
                    uint64_t cut = 0; bool unterminated = false;
                    rc = bw.step(w, true, carry, cut, unterminated, wn, err);
                    if (rc == 1) { say(wn); return 1; }
                    if (rc) { say(err); return code_of(Rc::DeviceNoParam, rc); }
                    if (cut) if (device_download(o + done, bw.text(w), (size_t)cut, err)) { say(err); return SHK_E_DEVICE; }
                    done += cut;
                }
                if (done != chain.text) { say("the windows do not add up"); return SHK_E_INTERNAL; }
                if (ms_total) *ms_total = now_ms() - t0;
                if (why) { msg.clear(); *why = msg.c_str(); }
                *out = o; *out_n = (size_t)done; o = nullptr;
                return SHK_OK;
            }
        }
        GpuText text; GpuInflateStats st;
        const int rc = gpu_inflate_member(gz, n, current_device(), nullptr, text, err, &st, true);
        if (why) { msg = rc == 1 ? st.why_not : err; *why = msg.c_str(); }
        if (ms_total) *ms_total = st.total_ms;
        if (rc == 1) return 1;
        if (rc) return code_of(Rc::DeviceNoParam, rc);
        const size_t bytes = text.e;
        uint8_t *o = (uint8_t *)malloc(bytes ? bytes : 1);
        if (!o) { gpu_text_free(text); return SHK_E_OOM; }
        const int rd = device_download(o, text.d, bytes, err);
        gpu_text_free(text);
        if (rd) { free(o); if (why) { msg = err; *why = msg.c_str(); } return SHK_E_DEVICE; }
        *out = o; *out_n = bytes;
        return SHK_OK;
    } catch (...) { return SHK_E_OOM; }
}
int shk_host_gunzip(const uint8_t *gz, size_t n, uint8_t **out, size_t *out_n, uint64_t *mt_members, double *reader_seconds) {
    try {
        if (!gz || !out || !out_n) return SHK_E_PARAM;
        ByteVec st; const uint8_t *p = nullptr; size_t pn = 0; std::string err;
        const double t0 = now_ms();
        const int rc = maybe_inflate(gz, n, st, p, pn, err);
        if (reader_seconds) *reader_seconds = (now_ms() - t0) * 1e-3;
        if (rc) return code_of(Rc::Inflater, rc);
        *out = (uint8_t *)malloc(pn ? pn : 1);
        if (!*out) return SHK_E_OOM;
        if (pn) memcpy(*out, p, pn);
        *out_n = pn;
        if (mt_members) *mt_members = inflate_mt_members();
        return SHK_OK;
    } catch (...) { return SHK_E_OOM; }
}
// the text of both unitig-graph entry points: "removed a b", then one line per contig, or "error: ..."
static char *unitig_assemble_text(bool on_device, uint32_t k, uint64_t n_recs, const uint64_t *first, const uint64_t *last, const uint64_t *len,
                                  const uint64_t *kc, const uint8_t *circ, const uint64_t *min_key, const uint8_t *min_o,
                                  const uint64_t *min_pos, int tips, int bubbles) {
    try {
        if ((k & 1u) == 0 || k < SHK_K_MIN || k > SHK_K_MAX || (n_recs && (!first || !last || !len || !kc || !circ))) return nullptr;
        const uint32_t W = (2 * k + 63) / 64;
        std::vector<UnitigRec> recs((size_t)n_recs);
        for (uint64_t r = 0; r < n_recs; r++) {
            for (uint32_t j = 0; j < W; j++) { recs[r].first[j] = first[r * W + j]; recs[r].last[j] = last[r * W + j]; }
            recs[r].len = len[r]; recs[r].kc = kc[r]; recs[r].circ = circ[r];
        }
        UnitigGraphResult res; std::string err;
        auto fail_text = [](const std::string &e) -> char * { const std::string t = "error: " + e; char *o = (char *)malloc(t.size() + 1); if (o) memcpy(o, t.c_str(), t.size() + 1); return o; };
        if (on_device) {
            // (1 — no device memory — is the caller's cue to run the host code: here it is reported, the caller asked for the device)
            const int rc = unitig_assemble_device((int)k, recs, tips != 0, bubbles != 0, current_device(), nullptr, res, err);
            if (rc == 1) return fail_text("out of device memory");
            if (rc) return fail_text(err);
        } else if (unitig_assemble((int)k, recs, tips != 0, bubbles != 0, res, err)) return fail_text(err);
        std::vector<UnitigMinKey> mk((size_t)n_recs);
        for (uint32_t r : res.need_min) {
            if (!min_key || !min_o || !min_pos) return nullptr;
            for (uint32_t j = 0; j < W; j++) mk[r].key[j] = min_key[(uint64_t)r * W + j];
            mk[r].o = min_o[r]; mk[r].pos = min_pos[r]; mk[r].valid = true;
        }
        if (unitig_resolve_rings((int)k, recs, mk, res, err)) return fail_text(err);
        std::string text = "removed " + std::to_string(res.tips_removed) + " " + std::to_string(res.bubbles_removed) + "\n";
        for (const UnitigFlatContig &c : res.lin) {                 // (the walk ran on the device: the linear contigs, then the rings)
            text += "0 0 " + std::to_string(c.len_nodes) + " " + std::to_string(c.kc) + " :";
            for (uint32_t i = 0; i < c.n_recs; i++) text += " " + std::to_string(res.recs_flat[c.rec_off + i]);
            text += "\n";
        }
        for (const UnitigContig &c : res.contigs) {
            text += std::to_string(c.ring ? 1 : 0) + " " + std::to_string(c.rot) + " " + std::to_string(c.len_nodes) + " " + std::to_string(c.kc) + " :";
            for (uint32_t r : c.recs) text += " " + std::to_string(r);
            text += "\n";
        }
        char *out = (char *)malloc(text.size() + 1);
        if (!out) return nullptr;
        memcpy(out, text.c_str(), text.size() + 1);
        return out;
    } catch (...) { return nullptr; }
}
char *shk_host_unitig_assemble(uint32_t k, uint64_t n_recs, const uint64_t *first, const uint64_t *last, const uint64_t *len,
                               const uint64_t *kc, const uint8_t *circ, const uint64_t *min_key, const uint8_t *min_o,
                               const uint64_t *min_pos, int tips, int bubbles) {
    return unitig_assemble_text(false, k, n_recs, first, last, len, kc, circ, min_key, min_o, min_pos, tips, bubbles);
}
char *shk_device_unitig_assemble(uint32_t k, uint64_t n_recs, const uint64_t *first, const uint64_t *last, const uint64_t *len,
                                 const uint64_t *kc, const uint8_t *circ, const uint64_t *min_key, const uint8_t *min_o,
                                 const uint64_t *min_pos, int tips, int bubbles) {
    return unitig_assemble_text(true, k, n_recs, first, last, len, kc, circ, min_key, min_o, min_pos, tips, bubbles);
}
// the text of both entry points of the S10 walk: one line per contig — "0 nodes kc text_offset : record@node_offset ..." for a
// linear one, "1 nodes kc - : record ..." for a ring —, then "need_min : record ...", or "error: ..."
static char *unitig_chains_text(bool on_device, uint32_t k, uint64_t n_recs, const uint64_t *first, const uint64_t *len, const uint64_t *kc,
                                const uint8_t *circ, const uint8_t *alive, const uint32_t *mirror, const uint32_t *succ) {
    try {
        if ((k & 1u) == 0 || k < SHK_K_MIN || k > SHK_K_MAX || (n_recs && (!first || !len || !kc || !circ || !alive || !mirror || !succ))) return nullptr;
        const uint32_t W = (2 * k + 63) / 64;
        std::vector<UnitigRec> recs((size_t)n_recs);
        for (uint64_t r = 0; r < n_recs; r++) {
            for (uint32_t j = 0; j < W; j++) recs[r].first[j] = first[r * W + j];
            recs[r].len = len[r]; recs[r].kc = kc[r]; recs[r].circ = circ[r];
        }
        std::vector<uint8_t> v_alive(alive, alive + n_recs);
        std::vector<uint32_t> v_mirror(mirror, mirror + n_recs), v_succ(succ, succ + n_recs);
        UnitigGraphResult res; std::string err;
        auto fail_text = [](const std::string &e) -> char * { const std::string t = "error: " + e; char *o = (char *)malloc(t.size() + 1); if (o) memcpy(o, t.c_str(), t.size() + 1); return o; };
        // (the same check in front of both: the kernels never see links that do not fit together)
        if (unitig_chains_check(recs, v_alive, v_mirror, v_succ, err)) return fail_text(err);
        std::string text;
        if (on_device) {
            const int rc = unitig_chains_device((int)k, recs, v_alive, v_mirror, v_succ, current_device(), nullptr, res, err);
            if (rc == 1) return fail_text("out of device memory");
            if (rc) return fail_text(err);
            if (!res.flat || res.place.size() != (size_t)n_recs) return fail_text("unitig chains: the device handed over no flat form");
            for (const UnitigFlatContig &c : res.lin) {
                text += "0 " + std::to_string(c.len_nodes) + " " + std::to_string(c.kc) + " " + std::to_string(c.text_off) + " :";
                for (uint32_t i = 0; i < c.n_recs; i++) {
                    const uint32_t r = res.recs_flat[c.rec_off + i];
                    text += " " + std::to_string(r) + "@" + std::to_string(res.place[r].node_off);
                }
                text += "\n";
            }
        } else if (unitig_chains((int)k, recs, v_alive, std::move(v_mirror), v_succ, res, err)) return fail_text(err);
        uint64_t text_off = 0;
        for (const UnitigContig &c : res.contigs) {
            if (c.ring) { text += "1 " + std::to_string(c.len_nodes) + " " + std::to_string(c.kc) + " - :"; for (uint32_t r : c.recs) text += " " + std::to_string(r); }
            else {
                text += "0 " + std::to_string(c.len_nodes) + " " + std::to_string(c.kc) + " " + std::to_string(text_off) + " :";
                uint64_t node_off = 0;
                for (uint32_t r : c.recs) { text += " " + std::to_string(r) + "@" + std::to_string(node_off); node_off += recs[r].len; }
                text_off += c.len_nodes + (uint64_t)(k - 1);
            }
            text += "\n";
        }
        text += "need_min :";
        for (uint32_t r : res.need_min) text += " " + std::to_string(r);
        text += "\n";
        char *out = (char *)malloc(text.size() + 1);
        if (!out) return nullptr;
        memcpy(out, text.c_str(), text.size() + 1);
        return out;
    } catch (...) { return nullptr; }
}
char *shk_host_unitig_chains(uint32_t k, uint64_t n_recs, const uint64_t *first, const uint64_t *len, const uint64_t *kc, const uint8_t *circ,
                             const uint8_t *alive, const uint32_t *mirror, const uint32_t *succ) {
    return unitig_chains_text(false, k, n_recs, first, len, kc, circ, alive, mirror, succ);
}
char *shk_device_unitig_chains(uint32_t k, uint64_t n_recs, const uint64_t *first, const uint64_t *len, const uint64_t *kc, const uint8_t *circ,
                               const uint8_t *alive, const uint32_t *mirror, const uint32_t *succ) {
    return unitig_chains_text(true, k, n_recs, first, len, kc, circ, alive, mirror, succ);
}

}  // extern "C"
