// block_cache.h — the bookkeeping of the process-wide device block cache (device_mem.hip), free of HIP: the device calls it
// makes (current device, allocate, free, and the test mode's fill) come in as a backend, so tests/cpp/pool_main.cpp runs it
// on malloc.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <atomic>
#include <map>
#include <memory>
#include <mutex>
#include <utility>

namespace shk {

// Peak device memory of a handle (the reference reports peak wasm memory with every assembly: Assembler.ts:69-71,137).
// Every block the cache hands out is charged to the accounting context the calling thread carries (set by the C ABI's entry
// points for the handle they serve) and released from the context it was charged to, whichever thread gives it back.
struct MemAcct {
    std::atomic<uint64_t> cur{0}, peak{0};
    void add(uint64_t b) { const uint64_t c = cur.fetch_add(b) + b; uint64_t p = peak.load(); while (c > p && !peak.compare_exchange_weak(p, c)) {} }
    void sub(uint64_t b) { cur.fetch_sub(b); }
};
inline thread_local std::shared_ptr<MemAcct> tls_mem_acct;

struct BlockBackend {
    int (*cur_dev)();
    int (*alloc)(void **p, size_t bytes);          // 0, or the device's error code (then *p stays null)
    void (*free)(void *p);
    void (*fill)(void *p, size_t bytes, uint32_t word) = nullptr;      // optional: every 32-bit word of [p, p + bytes) = word, done when it returns
};

// Cache of device allocations: a handle lives for one preprocess+assemble, and hipMalloc/hipFree of its multi-GB buffers
// cost more than the kernels (measured ~10 ms/step).  Blocks are returned here on release and reused by the next handle;
// trim() gives them back to the driver.  NO stream-ordering bookkeeping: a block that comes back is handed to whoever asks
// next, on any stream — whoever releases one makes sure first that nothing in flight touches it (device_mem.h).
struct BlockCache {
    const BlockBackend be;
    const bool enabled;                                            // false: put frees at once, get never reuses
    std::mutex mu;
    std::multimap<std::pair<int, size_t>, void *> free_blocks;     // (device, bytes) -> block
    struct Out { int dev; std::shared_ptr<MemAcct> acct; };
    std::map<void *, Out> owner_dev;                               // every block handed out -> the device it lives on, who pays for it
    // TEST MODE, off by default (shk_debug_pool_fill, SHK_POOL_FILL): a block is never cleared, so every buffer starts with what
    // its previous user left and has a tail nobody wrote.  With the mode on, get() fills the WHOLE block it hands out — the
    // rounded size, fresh and reused alike — with one word before it returns, which makes those contents an input a test
    // chooses.  Off costs one relaxed load per hand-out.
    std::atomic<uint64_t> fill_mode{0};                            // bit 32: on; bits 0..31: the word
    std::atomic<uint64_t> filled_bytes{0};                         // bytes filled so far, blocks and fill_outside() alike
    BlockCache(const BlockBackend &b, bool on) : be(b), enabled(on) {}
    int set_fill(bool on, uint32_t word) { return (int)(fill_mode.exchange((on ? (uint64_t)1 << 32 : 0) | word) >> 32); }      // the previous `on`
    // memory that does not come from the cache but is used like a block of it: filled by the same rule
    void fill_outside(void *p, size_t bytes) {
        const uint64_t f = fill_mode.load(std::memory_order_relaxed);
        if (!(f >> 32) || !be.fill || !p || !bytes) return;
        be.fill(p, bytes, (uint32_t)f);
        filled_bytes.fetch_add(bytes, std::memory_order_relaxed);
    }
    // bytes: rounded up to the block actually handed out; err: the backend's code when nullptr comes back
    void *get(size_t &bytes, int &err) {
        bytes = (bytes + 4095) & ~(size_t)4095;
        // big scratch buffers vary a little from handle to handle: round them up so the cached block fits again
        if (bytes > ((size_t)256 << 20)) bytes = (bytes + ((size_t)256 << 20) - 1) & ~(((size_t)256 << 20) - 1);
        const int dev = be.cur_dev();
        const std::shared_ptr<MemAcct> &acct = tls_mem_acct;
        void *p = nullptr;
        if (enabled) {
            std::lock_guard<std::mutex> lk(mu);
            auto it = free_blocks.lower_bound(std::make_pair(dev, bytes));
            if (it != free_blocks.end() && it->first.first == dev && it->first.second <= bytes + bytes / 2 + (1u << 20)) {
                p = it->second; bytes = it->first.second; free_blocks.erase(it); owner_dev[p] = Out{dev, acct}; err = 0;
                if (acct) acct->add(bytes);
            }
        }
        if (p) { fill_outside(p, bytes); return p; }      // (filled outside the lock: the fill waits for the device)
        err = be.alloc(&p, bytes);
        if (err && enabled) {                          // out of memory: drop the cache and retry once
            trim();
            err = be.alloc(&p, bytes);
        }
        if (!err) { std::lock_guard<std::mutex> lk(mu); owner_dev[p] = Out{dev, acct}; if (acct) acct->add(bytes); }
        if (!err) fill_outside(p, bytes);
        return !err ? p : nullptr;
    }
    // a block goes back under the device it was allocated on, whatever device the calling thread has current
    // (an FFI consumer may free a handle from another thread: the HIP current device is per thread)
    void put(void *p, size_t bytes) {
        if (!p) return;
        std::lock_guard<std::mutex> lk(mu);
        auto it = owner_dev.find(p);
        const int dev = it != owner_dev.end() ? it->second.dev : be.cur_dev();
        if (it != owner_dev.end()) { if (it->second.acct) it->second.acct->sub(bytes); owner_dev.erase(it); }
        if (!enabled) { be.free(p); return; }
        free_blocks.emplace(std::make_pair(dev, bytes), p);
    }
    void trim() {
        std::lock_guard<std::mutex> lk(mu);
        for (auto &kv : free_blocks) be.free(kv.second);
        free_blocks.clear();
    }
};

}  // namespace shk
