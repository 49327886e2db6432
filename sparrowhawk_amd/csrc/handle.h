// handle.h — what api.cpp, preprocess.cpp and shard_preprocess.cpp share: the handle behind the C ABI (include/shk.h), its call-order
// state, the guards an entry point runs under and the mapping of the library's internal return codes.
#pragma once
#include "../../include/shk.h"

#include <chrono>
#include <memory>
#include <string>

#include "fastq.h"
#include "outputs.h"
#include "device_mem.h"
#include "pipeline.h"
#include "shard_comm.h"

enum class St { Fresh, Streaming, Sharding, Preprocessed, Assembled, Failed };

inline double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct shk_handle {
    uint32_t k = 31, min_count = 5, min_qual = 20;
    uint64_t chunk_size = 0;
    bool verbose = false, do_bloom = false, do_fit = false, no_bubble = false, no_deadend = false;
    St st = St::Fresh;
    shk::IPipeline *pipe = nullptr;
    shk_progress_cb cb = nullptr;
    void *cb_user = nullptr;
    std::string err, first_err, pre_json, timings_json;
    shk::ByteVec asm_json;             // NUL-terminated
    const char *asm_json_dev = nullptr; // a fragmented assembly's JSON, written on the device: pinned memory owned by the pipeline
    uint64_t histo[SHK_HISTO_BINS] = {0};
    uint32_t used_min_count = 0;
    bool fit_ok = false;
    shk::PackedReads stream_reads;     // shk_push_reads accumulator
    uint64_t n_reads = 0;
    uint64_t batches_started = 0;      // batches handed to the pipeline (a failure after the first one poisons the handle)
    shk::ShardComm *shard_comm = nullptr;   // sharded assembly: the communicator shk_shard_preprocess ran on (shk_assemble is collective over it)
    shk::AssemblyText text;
    std::shared_ptr<void> mem = shk::mem_acct_new();   // device bytes this handle holds / held at most (device_mem.h: mem_acct_*)

    const char *mode() const { return do_bloom ? "bloom" : (chunk_size > 0 ? "chunked" : "bulk"); }
    void post(const std::string &s) { if (cb) cb(s.c_str(), cb_user); }
    void post_mode(const char *suffix) { post(std::string("preprocess:") + mode() + ":" + suffix); }
    // `loop:start` / `loop:end` exist for bulk and bloom only: the reference UI defines no such state for the
    // chunked mode (AssemblyPage.vue:548-579 has :start, :fitting, :filtering and :loop:<n>[:<pct>])
    void post_loop_edge(const char *suffix) { if (do_bloom || chunk_size == 0) post_mode(suffix); }
    void post_start() { post("preprocess:start"); post_mode("start"); post_loop_edge("loop:start"); }   // how every preprocess entry point opens
    uint64_t progress_every() const { return (!do_bloom && chunk_size > 0) ? chunk_size : 100000; }
};

inline int fail(shk_handle *h, int code, const std::string &msg) { h->err = msg; return code; }

// The internal return codes (< 0) of the four kinds of callee as SHK_E_* codes: the device layer (-4 memory, -1 a bad argument, else HIP), those
// of its calls whose -1 has always been reported as a device error, the host parser (-3 malformed, -4 memory) and the host inflater (-3 damaged).
enum class Rc { Device, DeviceNoParam, Parser, Inflater };
inline int code_of(Rc from, int rc) {
    if (from == Rc::Parser) return rc == -3 ? SHK_E_PARSE : (rc == -4 ? SHK_E_OOM : SHK_E_PARAM);
    if (from == Rc::Inflater) return rc == -3 ? SHK_E_PARSE : SHK_E_OOM;
    if (from == Rc::Device && rc == -1) return SHK_E_PARAM;
    return rc == -4 ? SHK_E_OOM : SHK_E_DEVICE;
}
inline int fail_rc(shk_handle *h, Rc from, int rc, const std::string &err) { return fail(h, code_of(from, rc), err); }

// Every entry point that touches the device runs with the HANDLE's device current (the HIP current device is
// per thread and new threads start on device 0: an FFI consumer may call from any thread) and restores the
// caller's device afterwards; no exception crosses the C ABI (shk.h: "never aborts").
struct DevGuard {
    int prev;
    explicit DevGuard(int dev) : prev(shk::set_device(dev)) {}
    ~DevGuard() { (void)shk::set_device(prev); }
    DevGuard(const DevGuard &) = delete;
    DevGuard &operator=(const DevGuard &) = delete;
};
// the calling thread allocates (and frees) device blocks on behalf of this handle while the guard lives
struct MemGuard {
    std::shared_ptr<void> prev;
    explicit MemGuard(const std::shared_ptr<void> &a) : prev(shk::mem_acct_set(a)) {}
    ~MemGuard() { (void)shk::mem_acct_set(prev); }
    MemGuard(const MemGuard &) = delete;
    MemGuard &operator=(const MemGuard &) = delete;
};
