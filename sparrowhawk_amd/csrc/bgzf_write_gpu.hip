// bgzf_write_gpu.hip — text in HBM as a finished BGZF file (bgzf_write_gpu.h; SPEC S11a).
//   k_json_unesc_count / k_json_unesc_write   JSON string content -> its bytes: a stream compaction (count, scan, write)
//   k_bgzf_encode                             one wave per block of 65 280 bytes: histogram + CRC-32, the plan of deflate_write.h,
//                                             the bits, into a slot of 64 KiB of its own
//   k_bgzf_gather                             the blocks back to back: header, deflate data (or the stored text), trailer; the end marker
#include <hip/hip_runtime.h>
#include <chrono>
#include <string.h>

#include "bgzf_write_gpu.h"
#include "deflate_write.h"
#include "device_mem.h"
#include "scan_gpu.h"

namespace shk {
namespace {

typedef unsigned long long u64;

// ---- JSON unescape -------------------------------------------------------------------------------------------------------
// A backslash BEGINS an escape pair where the run of backslashes in front of it is of even length; the pair becomes one byte.
// Every thread finds the state at the start of its 8 bytes by looking back in the text itself, so a pair may straddle any
// boundary (of a thread's bytes, of a chunk) at either of its bytes.  flags[0] |= 1: a pair that is none of \n \t \" \\, or a
// backslash that begins a pair at the last byte.
__device__ __forceinline__ bool pair_open_at(const uint8_t *__restrict__ src, u64 i) {      // is src[i] the second byte of a pair?
    u64 run = 0;
    while (i > run && src[i - 1 - run] == '\\') run++;
    return (run & 1ull) != 0;
}
__device__ __forceinline__ uint32_t unesc_char(uint32_t c, bool &ok) {
    ok = true;
    if (c == 'n') return '\n';
    if (c == 't') return '\t';
    if (c == '"' || c == '\\') return c;
    ok = false;
    return c;
}
// the pairs that begin in this thread's bytes (mask: bit j = byte j begins one)
__device__ __forceinline__ uint32_t unesc_scan8(const uint8_t *__restrict__ src, u64 n, u64 b, uint32_t &mask, bool &open, bool &bad) {
    mask = 0; bad = false; open = false;
    if (b >= n) return 0;
    bool st = pair_open_at(src, b);
    open = st;
    const u64 e = b + UNESC_PER_THREAD < n ? b + UNESC_PER_THREAD : n;
    uint32_t starts = 0;
    for (u64 i = b; i < e; i++) {
        const uint32_t c = src[i];
        if (st) { bool ok; (void)unesc_char(c, ok); bad |= !ok; st = false; }
        else if (c == '\\') { st = true; starts++; mask |= 1u << (uint32_t)(i - b); bad |= i + 1 == n; }
    }
    return starts;
}
__global__ __launch_bounds__(256) void k_json_unesc_count(const uint8_t *__restrict__ src, u64 n, u64 *__restrict__ cnt, uint32_t *__restrict__ flags) {
    __shared__ uint32_t wsum[4];
    const u64 b = (u64)blockIdx.x * UNESC_CHUNK + (u64)threadIdx.x * UNESC_PER_THREAD;
    uint32_t mask; bool open, bad;
    uint32_t v = unesc_scan8(src, n, b, mask, open, bad);
    if (bad) atomicOr(&flags[0], 1u);
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) cnt[blockIdx.x] = (u64)wsum[0] + wsum[1] + wsum[2] + wsum[3];
}
// off[chunk]: the pairs that begin in front of the chunk; byte i goes to i - (the pairs that begin in front of or at i)
__global__ __launch_bounds__(256) void k_json_unesc_write(const uint8_t *__restrict__ src, u64 n, const u64 *__restrict__ off, uint8_t *__restrict__ dst) {
    __shared__ uint32_t wsum[4];
    const u64 b = (u64)blockIdx.x * UNESC_CHUNK + (u64)threadIdx.x * UNESC_PER_THREAD;
    uint32_t mask; bool open, bad;
    const uint32_t mine = unesc_scan8(src, n, b, mask, open, bad);
    uint32_t incl = mine;
    const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    for (int o = 1; o < 64; o <<= 1) { const uint32_t u = __shfl_up(incl, o); if (lane >= (uint32_t)o) incl += u; }
    if (lane == 63) wsum[wid] = incl;
    __syncthreads();
    u64 before = off[blockIdx.x] + (incl - mine);
    for (uint32_t w = 0; w < wid; w++) before += wsum[w];
    if (b >= n) return;
    const u64 e = b + UNESC_PER_THREAD < n ? b + UNESC_PER_THREAD : n;
    bool second = open;
    for (u64 i = b; i < e; i++) {
        const uint32_t c = src[i];
        if (mask & (1u << (uint32_t)(i - b))) { before++; second = true; continue; }      // the backslash of a pair: dropped
        bool ok;
        dst[i - before] = (uint8_t)(second ? unesc_char(c, ok) : c);
        second = false;
    }
}

// ---- the block encoder ---------------------------------------------------------------------------------------------------
struct BlkOut { uint32_t bytes, crc, stored, pad; };      // bytes: the deflate data (a stored block: 5 + the text)
static constexpr uint32_t ENC_STAGE = 484;                // dwords: 31 bits carried + 64 lanes x 240 bits (480 dwords), and room for a spill-over
static constexpr uint32_t ENC_ROUND = 1024;               // bytes of text a round: 64 lanes x 16
struct EncLds {
    uint32_t hist[DW_LIT + 3];
    uint32_t crc_tab[4][256];
    DwScratch s;
    DwPlan p;
    uint32_t stage[ENC_STAGE];
};      // about 11 KiB a wave

// flags[1] |= 1: a block whose bits did not come out at the size its plan gave; flags[2] += the stored blocks
__global__ __launch_bounds__(64) void k_bgzf_encode(const uint8_t *__restrict__ text, u64 n, uint32_t n_blocks, uint32_t *__restrict__ slots,
                                                   BlkOut *__restrict__ out, u64 *__restrict__ sizes, uint32_t *__restrict__ flags) {
    __shared__ EncLds L;
    const uint32_t blk = blockIdx.x;
    if (blk >= n_blocks) return;
    const uint32_t lane = threadIdx.x;
    const u64 t0 = (u64)blk * DW_BLOCK_TEXT;
    const uint32_t nb = (uint32_t)(n - t0 < (u64)DW_BLOCK_TEXT ? n - t0 : (u64)DW_BLOCK_TEXT);
    const uint8_t *__restrict__ src = text + t0;
    const bool aligned = (reinterpret_cast<uintptr_t>(src) & 15u) == 0;
    for (uint32_t e = lane; e < DW_LIT + 3; e += 64) L.hist[e] = 0;
    for (uint32_t e = lane; e < ENC_STAGE; e += 64) L.stage[e] = 0;
    for (uint32_t e = lane; e < 256; e += 64) L.crc_tab[0][e] = dw_crc_entry(e);
    __syncthreads();
    for (uint32_t e = lane; e < 256; e += 64) {
        uint32_t cc = L.crc_tab[0][e];
        for (int t = 1; t < 4; t++) { cc = (cc >> 8) ^ L.crc_tab[0][cc & 0xFFu]; L.crc_tab[t][e] = cc; }
    }
    __syncthreads();
    // ---- histogram and CRC-32: a lane takes 1024 consecutive bytes; the lanes' checksums are joined by the polynomial's arithmetic
    const uint32_t p0 = lane * ENC_ROUND < nb ? lane * ENC_ROUND : nb, p1 = p0 + ENC_ROUND < nb ? p0 + ENC_ROUND : nb;
    uint32_t crc = 0xFFFFFFFFu, p = p0;
    if (aligned) {
        for (; p + 16 <= p1; p += 16) {
            const uint4 v = *reinterpret_cast<const uint4 *>(src + p);
            const uint32_t ws[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const uint32_t x = crc ^ ws[q];
                crc = L.crc_tab[3][x & 0xFFu] ^ L.crc_tab[2][(x >> 8) & 0xFFu] ^ L.crc_tab[1][(x >> 16) & 0xFFu] ^ L.crc_tab[0][x >> 24];
                atomicAdd(&L.hist[ws[q] & 0xFFu], 1u); atomicAdd(&L.hist[(ws[q] >> 8) & 0xFFu], 1u);
                atomicAdd(&L.hist[(ws[q] >> 16) & 0xFFu], 1u); atomicAdd(&L.hist[ws[q] >> 24], 1u);
            }
        }
    }
    for (; p < p1; p++) { const uint32_t c = src[p]; atomicAdd(&L.hist[c], 1u); crc = L.crc_tab[0][(crc ^ c) & 0xFFu] ^ (crc >> 8); }
    crc ^= 0xFFFFFFFFu;
    uint32_t part = p1 > p0 ? dw_gf_mul(dw_gf_x8n((u64)(nb - p1)), crc) : 0u;
    for (int o = 32; o; o >>= 1) part ^= __shfl_xor(part, o);
    const uint32_t crc_all = part;
    if (lane == 0) L.hist[DW_EOB] = 1;
    __syncthreads();
    // ---- the plan: ranks by all lanes, the serial part by one
    dw_rank(L.hist, DW_LIT, L.s.order, (int)lane, 64);
    __syncthreads();
    if (lane == 0) { dw_plan(L.hist, nb, L.s, L.p); if (!L.p.stored) (void)dw_put_header(L.p, L.stage); }
    __syncthreads();
    if (L.p.stored) {
        if (lane == 0) { out[blk] = BlkOut{DW_STORED_HEAD + nb, crc_all, 1u, 0u}; sizes[blk] = (u64)DW_BGZF_HEAD + DW_STORED_HEAD + nb + DW_BGZF_TAIL; atomicAdd(&flags[2], 1u); }
        return;
    }
    // ---- the bits.  The stage holds T bits from its bottom; whole dwords go out, the partial one is carried.
    uint32_t *__restrict__ outw = slots + (size_t)blk * (DW_SLOT / 4);
    uint32_t T = L.p.header_bits, wpos = 0;
    auto flush = [&]() {
        const uint32_t nd = T >> 5;
        for (uint32_t e = lane; e < nd; e += 64) if (wpos + e < DW_SLOT / 4) outw[wpos + e] = L.stage[e];
        const uint32_t carry = L.stage[nd];                   // (nd <= 480)
        __syncthreads();
        for (uint32_t e = lane; e < ENC_STAGE; e += 64) L.stage[e] = e == 0 ? carry : 0u;
        __syncthreads();
        wpos += nd; T &= 31u;
    };
    flush();
    auto or_bits = [&](uint32_t bitpos, uint64_t v, uint32_t bits) {
        if (!bits) return;
        const uint32_t i = bitpos >> 5, sh = bitpos & 31u;
        const uint64_t lo = v << sh;
        const uint32_t top = sh ? (uint32_t)(v >> (64u - sh)) : 0u;
        if ((uint32_t)lo) atomicOr(&L.stage[i], (uint32_t)lo);
        if ((uint32_t)(lo >> 32)) atomicOr(&L.stage[i + 1], (uint32_t)(lo >> 32));
        if (top) atomicOr(&L.stage[i + 2], top);
    };
    const uint32_t rounds = (nb + ENC_ROUND - 1) / ENC_ROUND;
    for (uint32_t r = 0; r < rounds; r++) {
        const uint32_t q0 = r * ENC_ROUND + lane * 16u;
        const uint32_t cnt = q0 < nb ? (nb - q0 < 16u ? nb - q0 : 16u) : 0u;
        uint32_t ws[4] = {0u, 0u, 0u, 0u};
        if (cnt == 16u && aligned) { const uint4 v = *reinterpret_cast<const uint4 *>(src + q0); ws[0] = v.x; ws[1] = v.y; ws[2] = v.z; ws[3] = v.w; }
        else {
#pragma unroll
            for (uint32_t i = 0; i < 16; i++) if (i < cnt) ws[i >> 2] |= (uint32_t)src[q0 + i] << (8u * (i & 3u));
        }
        uint64_t g[4]; uint32_t gb[4], mine = 0;
#pragma unroll
        for (uint32_t q = 0; q < 4; q++) {
            uint64_t acc = 0; uint32_t b = 0;
#pragma unroll
            for (uint32_t j = 0; j < 4; j++) if (q * 4 + j < cnt) { const uint32_t c = (ws[q] >> (8u * j)) & 0xFFu; acc |= (uint64_t)L.p.code[c] << b; b += L.p.len[c]; }
            g[q] = acc; gb[q] = b; mine += b;
        }
        uint32_t incl = mine;
        for (int o = 1; o < 64; o <<= 1) { const uint32_t u = __shfl_up(incl, o); if (lane >= (uint32_t)o) incl += u; }
        const uint32_t all = __shfl(incl, 63);
        uint32_t pos = T + incl - mine;
#pragma unroll
        for (uint32_t q = 0; q < 4; q++) { or_bits(pos, g[q], gb[q]); pos += gb[q]; }
        __syncthreads();
        T += all;
        flush();
    }
    const uint32_t eob = L.p.len[DW_EOB];
    if (lane == 0) { uint32_t t = T; dw_put(L.stage, t, L.p.code[DW_EOB], eob); }
    T += eob;
    __syncthreads();
    const uint32_t nd = (T + 31u) >> 5;
    if (lane < nd && wpos + lane < DW_SLOT / 4) outw[wpos + lane] = L.stage[lane];
    const uint32_t bytes = wpos * 4u + ((T + 7u) >> 3);
    if (lane == 0) {
        out[blk] = BlkOut{bytes, crc_all, 0u, 0u};
        sizes[blk] = (u64)DW_BGZF_HEAD + bytes + DW_BGZF_TAIL;
        if (bytes != L.p.huffman_bytes) atomicOr(&flags[1], 1u);
    }
}

// off: the exclusive scan of the blocks' sizes; workgroup n_blocks writes the end marker behind the last block
__global__ __launch_bounds__(256) void k_bgzf_gather(const uint8_t *__restrict__ text, u64 n, uint32_t n_blocks, const uint8_t *__restrict__ slots,
                                                    const BlkOut *__restrict__ out, const u64 *__restrict__ off, const u64 *__restrict__ d_total,
                                                    uint8_t *__restrict__ file) {
    const uint32_t blk = blockIdx.x, t = threadIdx.x;
    if (blk > n_blocks) return;
    if (blk == n_blocks) { if (t < DW_EOF_BYTES) file[d_total[0] + t] = dw_bgzf_eof_byte(t); return; }
    const BlkOut o = out[blk];
    const u64 t0 = (u64)blk * DW_BLOCK_TEXT;
    const uint32_t nb = (uint32_t)(n - t0 < (u64)DW_BLOCK_TEXT ? n - t0 : (u64)DW_BLOCK_TEXT);
    const uint32_t total = DW_BGZF_HEAD + o.bytes + DW_BGZF_TAIL;
    uint8_t *__restrict__ dst = file + off[blk];
    if (t < DW_BGZF_HEAD) dst[t] = dw_bgzf_head_byte(t, total);
    uint8_t *__restrict__ body = dst + DW_BGZF_HEAD;
    if (o.stored) {
        if (t < DW_STORED_HEAD) body[t] = t == 0 ? 1 : (t == 1 ? (uint8_t)(nb & 0xFFu) : (t == 2 ? (uint8_t)(nb >> 8) : (t == 3 ? (uint8_t)(~nb & 0xFFu) : (uint8_t)((~nb >> 8) & 0xFFu))));
        const uint8_t *__restrict__ s = text + t0;
        for (uint32_t i = t; i < nb; i += 256) body[DW_STORED_HEAD + i] = s[i];
    } else {
        const uint8_t *__restrict__ s = slots + (size_t)blk * DW_SLOT;
        for (uint32_t i = t; i < o.bytes; i += 256) body[i] = s[i];
    }
    if (t < DW_BGZF_TAIL) body[o.bytes + t] = t < 4 ? (uint8_t)(o.crc >> (8u * t)) : (uint8_t)(nb >> (8u * (t - 4u)));
}

double host_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct Events {
    hipEvent_t a = nullptr, b = nullptr; bool ok = false;
    explicit Events(bool on) { if (on) ok = hipEventCreate(&a) == hipSuccess && hipEventCreate(&b) == hipSuccess; }
    ~Events() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
};

}  // namespace

int gpu_bgzf_write_pinned(const uint8_t *d_src, uint64_t n, bool escaped, void *stream, bool timers, const std::function<int(std::string &)> *wait,
                          PinnedBuf &file, size_t &file_n, BgzfWriteStats &S, std::string &err) {
    hipStream_t st = (hipStream_t)stream;
    auto sync = [&]() -> int {
        if (wait && *wait) return (*wait)(err);
        HIPCHK(hipStreamSynchronize(st));
        return 0;
    };
    S = BgzfWriteStats();
    file_n = 0;
    PoolScope sc(stream, "BGZF writer");
    Events ev(timers);
    if (ev.ok) (void)hipEventRecord(ev.a, st);
    uint32_t *d_flags = sc.get<uint32_t>(4, err);
    u64 *d_total = sc.get<u64>(2, err);
    if (!d_flags || !d_total) return -4;
    HIPCHK(hipMemsetAsync(d_flags, 0, 16, st));
    uint32_t h_flags[4] = {0, 0, 0, 0};
    u64 h_total = 0;
    const uint8_t *d_text = d_src;
    uint64_t m = n;
    if (escaped && n) {
        const uint64_t chunks = (n + UNESC_CHUNK - 1) / UNESC_CHUNK;
        if (chunks > 0x7FFFFFFFull) { err = "BGZF writer: a text of 2^42 bytes or more"; return -1; }
        u64 *cnt = sc.get<u64>(chunks, err);
        uint8_t *d_plain = sc.get<uint8_t>(n + 32, err);
        if (!cnt || !d_plain) return -4;
        hipLaunchKernelGGL(k_json_unesc_count, dim3((unsigned)chunks), dim3(256), 0, st, d_src, (u64)n, cnt, d_flags);
        HIPCHK(hipGetLastError());
        if (int rc = exclusive_scan(cnt, chunks, d_total, st, sc, err)) return rc;
        hipLaunchKernelGGL(k_json_unesc_write, dim3((unsigned)chunks), dim3(256), 0, st, d_src, (u64)n, (const u64 *)cnt, d_plain);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&h_total, d_total, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(h_flags, d_flags, 16, hipMemcpyDeviceToHost, st));
        if (int rc = sync()) return rc;
        if (h_flags[0]) { err = "BGZF writer: a backslash in the JSON text that begins none of \\n \\t \\\" \\\\"; return -6; }
        m = n - h_total;
        d_text = d_plain;
    }
    const uint64_t nblk = dw_n_blocks(m);
    if (nblk > 0x7FFFFFF0ull) { err = "BGZF writer: 2^31 blocks or more"; return -1; }
    uint32_t *d_slots = sc.get<uint32_t>((size_t)nblk * (DW_SLOT / 4), err);
    BlkOut *d_out = sc.get<BlkOut>(nblk, err);
    u64 *d_sizes = sc.get<u64>(nblk, err);
    if (!d_slots || !d_out || !d_sizes) return -4;
    if (nblk) {
        hipLaunchKernelGGL(k_bgzf_encode, dim3((unsigned)nblk), dim3(64), 0, st, d_text, (u64)m, (uint32_t)nblk, d_slots, d_out, d_sizes, d_flags);
        HIPCHK(hipGetLastError());
    }
    if (int rc = exclusive_scan(d_sizes, nblk, d_total, st, sc, err)) return rc;
    HIPCHK(hipMemcpyAsync(&h_total, d_total, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(h_flags, d_flags, 16, hipMemcpyDeviceToHost, st));
    if (int rc = sync()) return rc;
    if (h_flags[1]) { err = "BGZF writer: a block did not come out at the size of its plan"; return -6; }
    const size_t bytes = (size_t)h_total + DW_EOF_BYTES;
    uint8_t *d_file = sc.get<uint8_t>(bytes, err);
    if (!d_file) return -4;
    if (int rc = file.alloc(bytes, err)) return rc;
    hipLaunchKernelGGL(k_bgzf_gather, dim3((unsigned)nblk + 1u), dim3(256), 0, st, d_text, (u64)m, (uint32_t)nblk, (const uint8_t *)d_slots, (const BlkOut *)d_out,
                       (const u64 *)d_sizes, (const u64 *)d_total, d_file);
    HIPCHK(hipGetLastError());
    if (ev.ok) (void)hipEventRecord(ev.b, st);
    const double t0 = host_ms();
    HIPCHK(hipMemcpyAsync(file.p, d_file, bytes, hipMemcpyDeviceToHost, st));
    if (int rc = sync()) return rc;
    S.d2h_ms = host_ms() - t0;
    if (ev.ok) { float ms = 0; if (hipEventElapsedTime(&ms, ev.a, ev.b) == hipSuccess) S.kernels_ms = ms; }
    S.text_bytes = m; S.file_bytes = bytes; S.blocks = nblk; S.stored_blocks = h_flags[2];
    file_n = bytes;
    return 0;
}

int gpu_bgzf_write_host_pinned(const uint8_t *src, uint64_t n, bool escaped, void *stream, bool timers, const std::function<int(std::string &)> *wait,
                               PinnedBuf &file, size_t &file_n, BgzfWriteStats &S, std::string &err) {
    PoolScope sc(stream, "BGZF writer: the text");
    uint8_t *d_src = sc.get<uint8_t>(n + 32, err);
    if (!d_src) return -4;
    if (n) HIPCHK(hipMemcpyAsync(d_src, src, n, hipMemcpyHostToDevice, (hipStream_t)stream));
    return gpu_bgzf_write_pinned(d_src, n, escaped, stream, timers, wait, file, file_n, S, err);
}

int gpu_bgzf_write_host(const uint8_t *src, uint64_t n, bool escaped, bool timers, std::vector<uint8_t> &file, BgzfWriteStats &S, std::string &err) {
    PinnedBuf pin; size_t bytes = 0;
    const int rc = gpu_bgzf_write_host_pinned(src, n, escaped, nullptr, timers, nullptr, pin, bytes, S, err);
    if (rc) return rc;
    file.assign((const uint8_t *)pin.p, (const uint8_t *)pin.p + bytes);
    return 0;
}

}  // namespace shk
