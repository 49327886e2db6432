// The bookkeeping of the device block pool (csrc/block_cache.h) and its two owners (csrc/device_mem.h: PoolBlock, PoolScope)
// on a backend of malloc / free with counters and a settable "current device", and the fill-on-hand-out test mode of the
// pool on a backend whose fill writes (or only notes) what it is asked for: no GPU, no HIP.  Built with
// -fsanitize=address,undefined by tests/test_device_pool_host.py; prints "ok" and returns 0, or names the line that failed.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <set>
#include <string>

#include "block_cache.h"
#include "device_mem.h"

using namespace shk;

static int g_checks = 0, g_failed = 0;
#define CHECK(cond)                                                                       \
    do {                                                                                  \
        g_checks++;                                                                       \
        if (!(cond)) { g_failed++; fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

// ---- the backend: malloc without a write (a 512 MiB block costs address space only), every call counted
static int g_dev = 0, g_refuse = 0;                     // g_refuse: the next so many allocations fail
static long g_allocs = 0, g_frees = 0;
static std::set<void *> g_live;
static int fake_cur_dev() { return g_dev; }
static int fake_alloc(void **p, size_t bytes) {
    if (g_refuse > 0) { g_refuse--; *p = nullptr; return 2; }
    *p = malloc(bytes);
    if (!*p) return 2;
    g_allocs++; g_live.insert(*p);
    return 0;
}
static void fake_free(void *p) { g_frees++; if (!g_live.erase(p)) { fprintf(stderr, "free of a block that is not live\n"); g_failed++; return; } free(p); }
static const BlockBackend FAKE{fake_cur_dev, fake_alloc, fake_free};

static void *get(BlockCache &c, size_t want, size_t *got = nullptr) {
    size_t b = want; int e = -1;
    void *p = c.get(b, e);
    CHECK((p != nullptr) == (e == 0));
    if (got) *got = b;
    return p;
}

static void test_rounding() {
    BlockCache c(FAKE, true);
    size_t b = 0;
    void *p = get(c, 1, &b); CHECK(b == 4096); c.put(p, b);
    p = get(c, 4097, &b); CHECK(b == 8192); c.put(p, b);
    p = get(c, (size_t)256 << 20, &b); CHECK(b == (size_t)256 << 20); c.put(p, b);      // (exactly 256 MiB: not "above")
    p = get(c, (size_t)300 << 20, &b); CHECK(b == (size_t)512 << 20); c.put(p, b);
    p = get(c, ((size_t)256 << 20) + 1, &b); CHECK(b == (size_t)512 << 20); c.put(p, b);  // (the cached 512 MiB block again)
    c.trim();
    CHECK(g_live.empty());
}

static void test_reuse() {
    BlockCache c(FAKE, true);
    size_t b = 0;
    // the smallest cached block that is large enough, and the caller is told the CACHED size
    void *p8 = get(c, 8192), *p12 = get(c, 12288), *p4 = get(c, 4096);
    c.put(p12, 12288); c.put(p8, 8192); c.put(p4, 4096);
    void *q = get(c, 5000, &b); CHECK(q == p8 && b == 8192);
    c.put(q, b);
    // a request of 4096: a cached block is taken up to 4096 + 2048 + 1 MiB = 1 054 720 bytes
    c.trim();
    void *in = get(c, 257 * 4096), *out = get(c, 258 * 4096);      // 1 052 672 and 1 056 768
    c.put(in, 257 * 4096);
    const long a0 = g_allocs;
    q = get(c, 4096, &b); CHECK(q == in && b == 257 * 4096 && g_allocs == a0);
    c.put(q, b);
    c.trim();
    c.put(out, 258 * 4096);
    q = get(c, 4096, &b); CHECK(q != out && b == 4096 && g_allocs == a0 + 1);
    c.put(q, b);
    c.trim();
    CHECK(g_live.empty());
}

static void test_devices() {
    BlockCache c(FAKE, true);
    g_dev = 1;
    void *p1 = get(c, 4096);
    c.put(p1, 4096);
    g_dev = 0;
    void *p0 = get(c, 4096); CHECK(p0 != p1);            // device 1's block is not device 0's
    g_dev = 1;
    void *q = get(c, 4096); CHECK(q == p1);
    g_dev = 0;
    c.put(q, 4096);                                       // back under device 1, though device 0 is current
    void *r = get(c, 4096); CHECK(r != p1);
    g_dev = 1;
    q = get(c, 4096); CHECK(q == p1);
    c.put(q, 4096); c.put(p0, 4096); c.put(r, 4096);
    g_dev = 0;
    c.trim();
    CHECK(g_live.empty());
}

static void test_accounting() {
    BlockCache c(FAKE, true);
    auto a = std::make_shared<MemAcct>(), o = std::make_shared<MemAcct>();
    tls_mem_acct = a;
    size_t b1 = 0, b2 = 0;
    void *p1 = get(c, 10000, &b1); CHECK(b1 == 12288 && a->cur == 12288 && a->peak == 12288);
    void *p2 = get(c, 4096, &b2); CHECK(a->cur == 16384 && a->peak == 16384);
    tls_mem_acct = o;                                     // another context current at put: released from the one charged
    c.put(p2, b2); CHECK(a->cur == 12288 && a->peak == 16384 && o->cur == 0 && o->peak == 0);
    tls_mem_acct = nullptr;                               // none current
    c.put(p1, b1); CHECK(a->cur == 0 && a->peak == 16384);
    void *u = get(c, 4096); CHECK(a->cur == 0 && o->cur == 0);      // no context: nobody pays
    c.put(u, 4096);
    tls_mem_acct = o;                                     // reuse charges the cached size
    size_t b3 = 0;
    void *p3 = get(c, 9000, &b3); CHECK(p3 == p1 && b3 == 12288 && o->cur == 12288 && o->peak == 12288);
    c.put(p3, b3); CHECK(o->cur == 0 && o->peak == 12288 && a->peak == 16384);
    tls_mem_acct = nullptr;
    c.trim();
    CHECK(g_live.empty());
}

static void test_refusals() {
    BlockCache c(FAKE, true);
    auto a = std::make_shared<MemAcct>();
    tls_mem_acct = a;
    void *p = get(c, 4096), *q = get(c, 8192);
    c.put(p, 4096); c.put(q, 8192);
    const long f0 = g_frees, a0 = g_allocs;
    g_refuse = 1;                                         // once: the cache is trimmed, the allocation retried
    size_t b = 0;
    void *r = get(c, 1 << 20, &b); CHECK(r && b == (1 << 20) && g_frees == f0 + 2 && g_allocs == a0 + 1 && g_refuse == 0 && a->cur == (1 << 20));
    CHECK(c.free_blocks.empty());
    c.put(r, b);
    g_refuse = 2;                                         // twice: nothing comes back, nothing is charged
    size_t want = 64 << 20; int e = 0;
    void *s = c.get(want, e); CHECK(!s && e != 0 && g_refuse == 0 && a->cur == 0 && c.owner_dev.empty());
    tls_mem_acct = nullptr;
    c.trim();
    CHECK(g_live.empty());
}

static void test_disabled() {
    BlockCache c(FAKE, false);
    const long f0 = g_frees, a0 = g_allocs;
    void *p = get(c, 4096);
    c.put(p, 4096); CHECK(g_frees == f0 + 1 && c.free_blocks.empty());
    void *q = get(c, 4096); CHECK(g_allocs == a0 + 2);    // (never reused)
    c.put(q, 4096); CHECK(g_frees == f0 + 2);
    g_refuse = 1;                                         // and a refusal is final: there is no cache to drop
    size_t want = 4096; int e = 0;
    CHECK(!c.get(want, e) && e != 0);
    CHECK(g_live.empty());
}

static void test_trim() {
    BlockCache c(FAKE, true);
    void *p[5];
    for (int i = 0; i < 5; i++) p[i] = get(c, (size_t)(i + 1) * 4096);
    for (int i = 0; i < 5; i++) c.put(p[i], (size_t)(i + 1) * 4096);
    const long f0 = g_frees;
    c.trim(); CHECK(g_frees == f0 + 5 && g_live.empty());
    c.trim(); CHECK(g_frees == f0 + 5);                   // every cached block exactly once
}

// ---- the fill-on-hand-out mode: a backend whose blocks are written by malloc's owner (0xA5 everywhere, so a byte the fill
// missed shows) and whose fill is counted
static long g_fills = 0; static uint64_t g_fill_bytes = 0;
static int dirty_alloc(void **p, size_t bytes) { const int e = fake_alloc(p, bytes); if (!e) memset(*p, 0xA5, bytes); return e; }
static void fake_fill(void *p, size_t bytes, uint32_t word) {
    g_fills++; g_fill_bytes += bytes;
    for (size_t i = 0; i < bytes; i++) ((unsigned char *)p)[i] = (unsigned char)(word >> (8 * (i & 3)));
}
static const BlockBackend DIRTY{fake_cur_dev, dirty_alloc, fake_free, fake_fill};
// a backend that never touches the memory: the fill notes what it was asked for
static void *g_noted_p = nullptr; static size_t g_noted_bytes = 0; static uint32_t g_noted_word = 0;
static void note_fill(void *p, size_t bytes, uint32_t word) { g_fills++; g_fill_bytes += bytes; g_noted_p = p; g_noted_bytes = bytes; g_noted_word = word; }
static const BlockBackend UNTOUCHED{fake_cur_dev, fake_alloc, fake_free, note_fill};

static bool all_words(const void *p, size_t bytes, uint32_t word) {
    for (size_t i = 0; i < bytes; i++) if (((const unsigned char *)p)[i] != (unsigned char)(word >> (8 * (i & 3)))) return false;
    return true;
}

static void test_fill() {
    const uint32_t W = 0x01020304u;                       // (four different bytes: a byte-wise fill in the wrong order shows)
    BlockCache c(DIRTY, true);
    size_t b = 0;
    const long f0 = g_fills; const uint64_t fb0 = g_fill_bytes;
    // off: the backend's fill is never called, nothing is counted
    void *p = get(c, 5000, &b); CHECK(b == 8192 && all_words(p, b, 0xA5A5A5A5u) && g_fills == f0 && c.filled_bytes == 0);
    c.put(p, b);
    void *q = get(c, 4097, &b); CHECK(q == p && g_fills == f0 && c.filled_bytes == 0);
    c.put(q, b);
    c.fill_outside(q, 16); CHECK(g_fills == f0 && all_words(q, 16, 0xA5A5A5A5u));
    c.trim();
    // on: the setter returns the previous state
    CHECK(c.set_fill(true, W) == 0 && c.set_fill(true, W) == 1);
    uint64_t handed = 0;
    // a fresh block, all of the rounded size
    const long a0 = g_allocs;
    p = get(c, 5000, &b); CHECK(g_allocs == a0 + 1 && b == 8192 && all_words(p, b, W)); handed += b;
    // a reused block of the same size, dirtied by its user meanwhile
    memset(p, 0x5A, b); c.put(p, b);
    q = get(c, 8192, &b); CHECK(q == p && g_allocs == a0 + 1 && b == 8192 && all_words(q, b, W)); handed += b;
    c.put(q, b);
    // a reused larger block: its tail beyond the bytes asked for is filled too
    void *big = get(c, 3 << 20, &b); CHECK(b == (3u << 20)); handed += b;
    memset(big, 0x5A, b); c.put(big, b);
    q = get(c, (2 << 20) + 1, &b); CHECK(q == big && b == (3u << 20) && all_words(q, b, W)); handed += b;
    c.put(q, b);
    // another word takes effect at the next hand-out
    CHECK(c.set_fill(true, 0xFFFFFFFFu) == 1);
    q = get(c, 100, &b); CHECK(b == 8192 && all_words(q, b, 0xFFFFFFFFu)); handed += b;
    c.put(q, b);
    CHECK(c.set_fill(true, W) == 1);
    // the retry after trim(): the first allocation is refused, the cache dropped, the second block filled
    const long fr0 = g_frees;
    g_refuse = 1;
    p = get(c, 64 << 10, &b); CHECK(p && b == (64u << 10) && g_frees > fr0 && c.free_blocks.empty() && all_words(p, b, W)); handed += b;
    c.put(p, b);
    // a refusal that stays one fills nothing
    const long f1 = g_fills;
    g_refuse = 2;
    size_t want = 1 << 20; int e = 0;
    CHECK(!c.get(want, e) && e != 0 && g_fills == f1);
    // memory from outside the cache, by the same rule: the bytes given, no rounding
    unsigned char outside[24]; memset(outside, 0xA5, sizeof outside);
    c.fill_outside(outside, 10); CHECK(all_words(outside, 10, W) && all_words(outside + 12, 12, 0xA5A5A5A5u) && outside[10] == 0xA5 && outside[11] == 0xA5);
    c.fill_outside(nullptr, 8); c.fill_outside(outside, 0);
    CHECK(c.filled_bytes == handed + 10 && g_fill_bytes - fb0 == handed + 10);
    // off again: the previous state comes back, and nothing more is filled or counted
    CHECK(c.set_fill(false, 0) == 1 && c.set_fill(false, 0) == 0);
    const long f2 = g_fills;
    p = get(c, 64 << 10, &b); memset(p, 0x5A, b); c.put(p, b);
    q = get(c, 64 << 10, &b); CHECK(q == p && all_words(q, b, 0x5A5A5A5Au) && g_fills == f2 && c.filled_bytes == handed + 10);
    c.put(q, b);
    c.trim();
    CHECK(g_live.empty());
    // a disabled cache (SHK_NO_POOL) fills its fresh blocks all the same
    {
        BlockCache d(DIRTY, false);
        d.set_fill(true, W);
        p = get(d, 1, &b); CHECK(b == 4096 && all_words(p, b, W) && d.filled_bytes == 4096);
        d.put(p, b);
    }
    // a backend without a fill: the mode is accepted and does nothing
    {
        BlockCache n(FAKE, true);
        n.set_fill(true, W);
        p = get(n, 1, &b); CHECK(p && n.filled_bytes == 0);
        n.put(p, b); n.trim();
    }
    CHECK(g_live.empty());
}

// above 256 MiB the rounded size is what is filled (memory never touched: address space only)
static void test_fill_large() {
    BlockCache c(UNTOUCHED, true);
    c.set_fill(true, 7);
    size_t b = 0;
    void *p = get(c, ((size_t)256 << 20) + 1, &b);
    CHECK(b == (size_t)512 << 20 && g_noted_p == p && g_noted_bytes == b && g_noted_word == 7 && c.filled_bytes == b);
    c.put(p, b);
    g_noted_p = nullptr;
    void *q = get(c, (size_t)400 << 20, &b);              // the cached 512 MiB block again: filled whole again
    CHECK(q == p && b == (size_t)512 << 20 && g_noted_p == p && g_noted_bytes == b && c.filled_bytes == 2 * b);
    c.put(q, b);
    c.trim();
    CHECK(g_live.empty());
}

// ---- the owners, over a pool of this backend
static BlockCache g_pool(FAKE, true);
static long g_releases = 0, g_syncs = 0;
namespace shk {
void *device_pool_alloc(size_t &bytes, int *hip_error) { int e = 0; void *p = g_pool.get(bytes, e); if (hip_error) *hip_error = e; return p; }
void device_pool_release(void *p, size_t bytes) { g_releases++; g_pool.put(p, bytes); }
int device_stream_sync(void *, std::string &) { g_syncs++; return 0; }
}  // namespace shk

static void test_pool_block() {
    long r0 = g_releases;
    { PoolBlock b; CHECK(b.get(0) && b.bytes == 4096 && b.as<char>() == (char *)b.p); }      // (0 bytes asks for 8)
    CHECK(g_releases == r0 + 1);
    void *taken; size_t taken_bytes;
    { PoolBlock b; CHECK(b.get(5000)); taken = b.take(); taken_bytes = b.bytes; CHECK(!b.p && taken_bytes == 8192); }
    CHECK(g_releases == r0 + 1);                          // take() leaves nothing to release
    { PoolBlock adopted(taken, taken_bytes); }
    CHECK(g_releases == r0 + 2);
    {
        PoolBlock a; CHECK(a.get(4096));
        PoolBlock b(std::move(a)); CHECK(!a.p && b.p);
        PoolBlock c; c = std::move(b); CHECK(!b.p && c.p);
    }
    CHECK(g_releases == r0 + 3);                          // a moved-from block releases nothing
    { PoolBlock b; CHECK(b.get(4096)); b.put(); b.put(); CHECK(!b.p); }
    CHECK(g_releases == r0 + 4);                          // put() twice releases once
    { PoolBlock b; }
    CHECK(g_releases == r0 + 4);
    CHECK(g_pool.owner_dev.empty());
}

static void test_pool_scope() {
    std::string err;
    long r0 = g_releases; int drains = 0; long releases_at_drain = -1;
    auto hook = [&] { drains++; releases_at_drain = g_releases; };
    { PoolScope sc(hook); }
    CHECK(drains == 0 && g_releases == r0);               // holds nothing: no drain
    void *kept; size_t kept_bytes;
    {
        PoolScope sc(hook);
        uint32_t *a = sc.get<uint32_t>(1000, err); uint64_t *b = sc.get<uint64_t>(0, err); char *k = sc.get<char>(9000, err);
        CHECK(a && b && k && err.empty());
        kept = k; kept_bytes = sc.keep(k); CHECK(kept_bytes == 12288 && sc.keep(k) == 0);
        CHECK(drains == 0 && g_releases == r0);
    }
    CHECK(drains == 1 && releases_at_drain == r0 && g_releases == r0 + 2);      // drained before the first release, once; the kept block stays out
    CHECK(g_pool.owner_dev.size() == 1 && g_pool.owner_dev.count(kept));
    device_pool_release(kept, kept_bytes);
    r0 = g_releases; drains = 0;
    {
        PoolScope sc(hook);
        char *a = sc.get<char>(100, err), *b = sc.get<char>(100, err);
        sc.release(a); CHECK(g_releases == r0 + 1 && drains == 0);             // the early hand-back does not drain
        sc.release(a); sc.release(nullptr); CHECK(g_releases == r0 + 1);
        (void)b;
    }
    CHECK(drains == 1 && g_releases == r0 + 2);
    const long s0 = g_syncs;
    { PoolScope sc((void *)nullptr, "test"); CHECK(sc.get<char>(1, err)); }     // a stream: the scope waits for it
    CHECK(g_syncs == s0 + 1);
    { PoolScope sc((void *)nullptr, "test"); g_refuse = 2; CHECK(!sc.get<char>(1 << 24, err) && err == "device allocation failed (test)"); }
    CHECK(g_syncs == s0 + 1);
    CHECK(g_pool.owner_dev.empty());
    g_pool.trim();
}

int main() {
    test_rounding();
    test_reuse();
    test_devices();
    test_accounting();
    test_refusals();
    test_disabled();
    test_trim();
    test_fill();
    test_fill_large();
    test_pool_block();
    test_pool_scope();
    CHECK(g_live.empty() && g_allocs == g_frees);         // the counters balance
    if (g_failed) { fprintf(stderr, "%d of %d checks failed\n", g_failed, g_checks); return 1; }
    printf("ok: %d checks\n", g_checks);
    return 0;
}
