// device_mem.hip — the process-wide device block pool over HIP, what parks on it (DeferScope), the stream cache and the small
// device / copy helpers (device_mem.h).  Host code only: no kernel lives here.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <map>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "block_cache.h"
#include "device_mem.h"
#include "pipeline.h"

namespace shk {

std::shared_ptr<void> mem_acct_new() { return std::static_pointer_cast<void>(std::make_shared<MemAcct>()); }
std::shared_ptr<void> mem_acct_set(std::shared_ptr<void> a) {
    std::shared_ptr<void> prev = std::static_pointer_cast<void>(tls_mem_acct);
    tls_mem_acct = std::static_pointer_cast<MemAcct>(a);
    return prev;
}
uint64_t mem_acct_peak(const std::shared_ptr<void> &a) { return a ? std::static_pointer_cast<MemAcct>(a)->peak.load() : 0; }
uint64_t mem_acct_current(const std::shared_ptr<void> &a) { return a ? std::static_pointer_cast<MemAcct>(a)->cur.load() : 0; }
void mem_acct_replay(const int64_t *deltas, size_t n, uint64_t *peak, uint64_t *current) {
    MemAcct a;
    for (size_t i = 0; i < n; i++) { if (deltas[i] >= 0) a.add((uint64_t)deltas[i]); else a.sub((uint64_t)(-deltas[i])); }
    if (peak) *peak = a.peak.load();
    if (current) *current = a.cur.load();
}

int current_device() { int d = 0; (void)hipGetDevice(&d); return d; }
int set_device(int dev) { int prev = 0; (void)hipGetDevice(&prev); if (prev != dev) (void)hipSetDevice(dev); return prev; }
int device_count() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// The fill of the pool's test mode (block_cache.h).  The null stream, then a wait for the WHOLE device: the library owns
// hipStreamNonBlocking streams (fastq_gpu.hip, inflate_gpu.hip, the copy stream), which the null stream does not order itself
// against, and the pool does not know which stream will use the block.  So this mode serialises the handles of a process: it
// shows a result that depends on stale memory, it does not show races.  (A tail of bytes % 4 exists only outside the pool.)
static void hip_fill(void *p, size_t bytes, uint32_t word) {
    if (bytes / 4) (void)hipMemsetD32Async((hipDeviceptr_t)p, (int)word, bytes / 4, nullptr);
    for (size_t i = bytes & ~(size_t)3; i < bytes; i++) (void)hipMemsetD8Async((hipDeviceptr_t)((char *)p + i), (unsigned char)(word >> (8 * (i & 3))), 1, nullptr);
    (void)hipDeviceSynchronize();
}
static BlockCache &dev_pool() {               // never destroyed (HIP teardown order); SHK_NO_POOL=1 and SHK_POOL_FILL are read once
    static BlockCache *p = [] {
        const char *v = getenv("SHK_NO_POOL");
        const BlockBackend hip{current_device, [](void **q, size_t bytes) { return (int)hipMalloc(q, bytes); }, [](void *q) { (void)hipFree(q); }, hip_fill};
        BlockCache *c = new BlockCache(hip, !(v && *v == '1'));
        const char *f = getenv("SHK_POOL_FILL");          // <hex word>: the test mode is on from the start (rank workers, tools)
        if (f && *f) {
            char *end = nullptr;
            const unsigned long long w = strtoull(f, &end, 16);
            if (end != f && !*end && w <= 0xFFFFFFFFull) c->set_fill(true, (uint32_t)w);
        }
        return c;
    }();
    return *p;
}
int device_pool_fill(bool on, uint32_t word) { return dev_pool().set_fill(on, word); }
uint64_t device_pool_filled_bytes() { return dev_pool().filled_bytes.load(); }
void device_fill_outside_pool(void *p, size_t bytes) { dev_pool().fill_outside(p, bytes); }
void device_pool_trim() { dev_pool().trim(); }
void *device_pool_alloc(size_t &bytes, int *hip_error) {
    int e = 0;
    void *p = dev_pool().get(bytes, e);
    if (hip_error) *hip_error = e;
    return p;
}
void device_pool_release(void *p, size_t bytes) { dev_pool().put(p, bytes); }

static thread_local std::vector<std::pair<void *, size_t>> *tls_defer = nullptr;
bool device_pool_park(void *p, size_t bytes) {
    if (!tls_defer) return false;
    try { tls_defer->push_back(std::make_pair(p, bytes)); return true; }
    catch (...) { return false; }                          // (no room for the note: the caller gives the block back now)
}
DeferScope::DeferScope(IPipeline *pipe) : pipe_(pipe) {
    auto *v = new (std::nothrow) std::vector<std::pair<void *, size_t>>();
    if (v) { try { v->reserve(256); } catch (...) {} }
    list_ = v; prev_ = tls_defer; tls_defer = v;
}
DeferScope::~DeferScope() {
    auto *v = (std::vector<std::pair<void *, size_t>> *)list_;
    tls_defer = (std::vector<std::pair<void *, size_t>> *)prev_;
    if (!v) return;
    if (!v->empty()) {
        if (pipe_) pipe_->drain();                        // nothing in flight reads or writes the parked blocks any more
        else (void)hipDeviceSynchronize();
        for (auto &b : *v) dev_pool().put(b.first, b.second);
    }
    delete v;
}

static std::mutex g_stream_mu;
static std::multimap<int, hipStream_t> &stream_cache() { static auto *c = new std::multimap<int, hipStream_t>(); return *c; }
hipStream_t stream_pool_get(int dev) {
    std::lock_guard<std::mutex> lk(g_stream_mu);
    auto it = stream_cache().find(dev);
    if (it == stream_cache().end()) return nullptr;
    hipStream_t s = it->second; stream_cache().erase(it); return s;
}
void stream_pool_put(int dev, hipStream_t s) {
    {
        std::lock_guard<std::mutex> lk(g_stream_mu);
        if (stream_cache().size() < 32) { stream_cache().emplace(dev, s); return; }
    }
    (void)hipStreamDestroy(s);
}

std::mutex &upload_token(int dev) { static std::mutex m[16]; return m[(unsigned)dev % 16u]; }

int device_upload(const void *host, size_t bytes, void **dptr, std::string &err) {
    *dptr = nullptr;
    HIPCHK(hipMalloc(dptr, bytes ? bytes : 4));
    device_fill_outside_pool(*dptr, bytes ? bytes : 4);
    if (bytes) {
        hipError_t e = hipMemcpy(*dptr, host, bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) { (void)hipFree(*dptr); *dptr = nullptr; err = hipGetErrorString(e); return -5; }
    }
    return 0;
}
void device_free(void *dptr) { if (dptr) (void)hipFree(dptr); }
int device_download(void *host, const void *dptr, size_t bytes, std::string &err) {
    HIPCHK(hipMemcpy(host, dptr, bytes, hipMemcpyDeviceToHost));
    return 0;
}
int device_stream_sync(void *stream, std::string &err) { HIPCHK(hipStreamSynchronize((hipStream_t)stream)); return 0; }
int device_copy_h2d_async(void *dst, const void *src, size_t bytes, void *stream, std::string &err) {
    if (bytes) HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
    return 0;
}

}  // namespace shk
