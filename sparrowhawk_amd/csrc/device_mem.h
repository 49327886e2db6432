// device_mem.h — device memory of the library (device_mem.hip): the process-wide block pool and its two owners, peak-memory
// accounting per handle, and the small device / copy helpers of the g++-compiled files (streams are void * here).
//
// THE RELEASE RULE.  The pool has no stream-ordering bookkeeping: a block that goes back is handed to whoever asks next, on
// any stream.  Whoever releases a block makes sure first that nothing in flight still touches it.  Three owners do that:
//   PoolBlock   one block; the code that holds it waits for its stream before the block dies.
//   PoolScope   a group of blocks used on one stream; its destructor drains that stream, THEN releases what it holds.
//   DevBuf<T>   Pipeline<W>'s typed buffers (HIP only, below): one that dies inside an entry point of the C ABI is parked
//               until DeferScope has drained the handle's stream — and stays charged to the handle until then.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <functional>
#include <memory>
#include <string>
#include <utility>
#include <vector>

namespace shk {

class IPipeline;              // pipeline.h

int device_count();
int current_device();          // the calling thread's current HIP device
int set_device(int dev);       // makes `dev` current for the calling thread, returns the previous one

// upload helper used by the host-buffer entry points
int device_upload(const void *host, size_t bytes, void **dptr, std::string &err);
void device_free(void *dptr);
int device_stream_sync(void *stream, std::string &err);      // waits for a hipStream_t
int device_copy_h2d_async(void *dst, const void *src, size_t bytes, void *stream, std::string &err);
int device_download(void *host, const void *dptr, size_t bytes, std::string &err);      // blocking device -> host copy

// the process-wide device block cache (block_cache.h): bytes is rounded up to the block actually handed out; hip_error,
// where asked for: the hipError_t of a failed allocation.  Outside this module only PoolBlock, PoolScope and DevBuf call these
// (and gpu_text_free / gpu_packed_free, for the plain records a block was handed over to).
void *device_pool_alloc(size_t &bytes, int *hip_error = nullptr);
void device_pool_release(void *p, size_t bytes);
void device_pool_trim();
// test mode of the pool (block_cache.h; shk_debug_pool_fill): on, every block is filled with `word`, all of it, when it is
// handed out.  device_pool_fill returns the previous `on`.  device_fill_outside_pool: for the two device allocations that do
// not come from the pool (device_upload, the communicator's stage buffer) — filled by the same rule, nothing when off.
int device_pool_fill(bool on, uint32_t word);
uint64_t device_pool_filled_bytes();
void device_fill_outside_pool(void *p, size_t bytes);

// peak device memory per handle (Assembler.ts:69-71,137 reports peak wasm memory with every assembly): an accounting context
// is made per handle, carried by the thread that serves it (mem_acct_set returns the previous one), and every block the pool
// hands out meanwhile is charged to it until it goes back
std::shared_ptr<void> mem_acct_new();
std::shared_ptr<void> mem_acct_set(std::shared_ptr<void> a);
uint64_t mem_acct_peak(const std::shared_ptr<void> &a);
uint64_t mem_acct_current(const std::shared_ptr<void> &a);
// the counter alone, on the host (tests): applies signed byte deltas, returns the high-water mark and what is left
void mem_acct_replay(const int64_t *deltas, size_t n, uint64_t *peak, uint64_t *current);

// One block of the pool, move-only; goes back when it dies.
struct PoolBlock {
    void *p = nullptr; size_t bytes = 0;
    PoolBlock() = default;
    PoolBlock(void *block, size_t block_bytes) : p(block), bytes(block_bytes) {}      // adopts a block of the pool (a GpuText's, given up)
    PoolBlock(const PoolBlock &) = delete;
    PoolBlock &operator=(const PoolBlock &) = delete;
    PoolBlock(PoolBlock &&o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; }
    PoolBlock &operator=(PoolBlock &&o) noexcept { if (this != &o) { put(); p = o.p; bytes = o.bytes; o.p = nullptr; } return *this; }
    ~PoolBlock() { put(); }
    bool get(size_t b) { put(); bytes = b ? b : 8; p = device_pool_alloc(bytes); return p != nullptr; }      // (the pool may hand out more: bytes says what)
    void put() { if (p) device_pool_release(p, bytes); p = nullptr; }
    void *take() { void *q = p; p = nullptr; return q; }      // the block is the caller's now (bytes still says how large)
    template <class T> T *as() const { return (T *)p; }
};

// Blocks of the pool used on ONE stream, returned on scope exit: the destructor first drains, then releases everything it
// still holds — an early error return may leave kernels in flight, and the order of the caller's locals does not matter.
// It drains only if it was ever asked for a block.  drain: the stream (hipStreamSynchronize), or a callable (the shard layer's watchdog).
class PoolScope {
  public:
    explicit PoolScope(void *stream, const char *what = nullptr) : drain_([stream] { std::string e; (void)device_stream_sync(stream, e); }), what_(what) {}
    explicit PoolScope(std::function<void()> drain, const char *what = nullptr) : drain_(std::move(drain)), what_(what) {}
    PoolScope(const PoolScope &) = delete;
    PoolScope &operator=(const PoolScope &) = delete;
    ~PoolScope() {
        if (!blocks_.empty()) drain_();
        for (auto &b : blocks_) if (b.first) device_pool_release(b.first, b.second);
    }
    // count == 0 asks for one element; nullptr: err says "device allocation failed (<what>)"
    template <typename T> T *get(size_t count, std::string &err) {
        size_t bytes = (count ? count : 1) * sizeof(T);
        void *p = device_pool_alloc(bytes);
        if (!p) { err = std::string("device allocation failed") + (what_ ? std::string(" (") + what_ + ")" : std::string()); return nullptr; }
        blocks_.emplace_back(p, bytes);
        return (T *)p;
    }
    // the block leaves the group (it is the caller's now); returns its size in the pool
    size_t keep(void *p) { for (auto &b : blocks_) if (b.first == p) { b.first = nullptr; return b.second; } return 0; }
    // early hand-back, for a site that knows the stream is idle there
    void release(void *p) { if (p) if (const size_t bytes = keep(p)) device_pool_release(p, bytes); }
  private:
    std::vector<std::pair<void *, size_t>> blocks_;
    std::function<void()> drain_;
    const char *what_;
};

// Device buffers (DevBuf) that go out of scope on the calling thread while this object lives are kept until it dies; then the
// pipeline's stream is drained and they go back to the pool.  One per entry point of the C ABI.
class DeferScope {
public:
    explicit DeferScope(IPipeline *pipe);
    ~DeferScope();
    DeferScope(const DeferScope &) = delete;
    DeferScope &operator=(const DeferScope &) = delete;
private:
    IPipeline *pipe_; void *list_; void *prev_;
};
// parks a block on the calling thread's DeferScope; false: there is none (or no room for the note)
bool device_pool_park(void *p, size_t bytes);

}  // namespace shk

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#include <map>
#include <mutex>

namespace shk {

// A failed HIP call inside a function with `err` in scope: err = "<text>: <hip string>", on_fail runs, -5 is returned.
#define HIPCHK_AS(text, call, on_fail)                                                    \
    do {                                                                                  \
        const hipError_t _e = (call);                                                     \
        if (_e != hipSuccess) {                                                           \
            err = std::string(text ": ") + hipGetErrorString(_e);                         \
            on_fail;                                                                      \
            return -5;                                                                    \
        }                                                                                 \
    } while (0)
#define HIPCHK(call) HIPCHK_AS(#call, call, (void)0)

// The typed, PARKING owner of Pipeline<W>'s members and locals.  A DevBuf that goes out of scope while an entry point of the
// C ABI runs is parked until that entry point has drained the handle's stream (DeferScope): an early `return rc` may destroy
// buffers that kernels, collectives or copies still in flight use, and the pool hands a freed block to whichever handle asks
// next (two handles in flight: batch.py).  Explicit release() calls — made where the code knows the stream is idle — go to
// the pool at once.
template <typename T> struct DevBuf {
    T *p = nullptr; size_t n = 0; size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() {
        if (p && device_pool_park(p, bytes)) { p = nullptr; n = 0; bytes = 0; return; }
        release();
    }
    void swap(DevBuf &o) { std::swap(p, o.p); std::swap(n, o.n); std::swap(bytes, o.bytes); }
    void release() { if (p) { device_pool_release(p, bytes); p = nullptr; n = 0; bytes = 0; } }
    int alloc(size_t count, std::string &err) {
        release();
        if (count == 0) count = 1;
        size_t b = count * sizeof(T);
        int e = 0;
        p = (T *)device_pool_alloc(b, &e);
        if (!p) { err = std::string("hipMalloc: ") + hipGetErrorString((hipError_t)e); return -4; }
        n = count; bytes = b; return 0;
    }
};

// pinned host staging buffer (D2H of contigs at full PCIe rate), cached the same way
struct PinnedBuf {
    char *p = nullptr; size_t bytes = 0;
    static std::mutex &mu() { static std::mutex m; return m; }
    static std::multimap<size_t, void *> &cache() { static auto *c = new std::multimap<size_t, void *>(); return *c; }
    ~PinnedBuf() { if (p) { std::lock_guard<std::mutex> lk(mu()); cache().emplace(bytes, p); } }
    int alloc(size_t b, std::string &err) {
        b = (b + 4095) & ~(size_t)4095; if (!b) b = 4096;
        if (p && bytes >= b) return 0;
        if (p) { std::lock_guard<std::mutex> lk(mu()); cache().emplace(bytes, p); p = nullptr; bytes = 0; }
        {
            std::lock_guard<std::mutex> lk(mu());
            auto it = cache().lower_bound(b);
            if (it != cache().end() && it->first <= 2 * b + (1u << 20)) { p = (char *)it->second; bytes = it->first; cache().erase(it); return 0; }
        }
        hipError_t e = hipHostMalloc((void **)&p, b, hipHostMallocDefault);
        if (e != hipSuccess) { p = nullptr; err = std::string("hipHostMalloc: ") + hipGetErrorString(e); return -4; }
        bytes = b; return 0;
    }
};

// streams of freed handles are reused too (create + destroy cost ~0.2 ms per handle); every use of a
// handle's stream ends in a synchronize, so a pooled stream is idle
// (key: device, or device + 1000 for the copy streams of the host-buffer entry points — creating and destroying one per
// handle cost ~1 ms of the 5.7 ms a step from host pinned memory took: profiles/r04)
hipStream_t stream_pool_get(int dev);          // nullptr: none cached
void stream_pool_put(int dev, hipStream_t s);

std::mutex &upload_token(int dev);

}  // namespace shk
#endif  // __HIPCC__
