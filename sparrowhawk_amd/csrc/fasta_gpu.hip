// fasta_gpu.hip — FASTA text -> segmented, 2-bit packed reads, on the device (SPEC S1a; fasta_gpu.h).
//
// The FASTQ parser (fastq_gpu.hip) gives a wave to every record.  A FASTA record may be a genome — millions of bases over
// lines of 60 or 80 characters — so this packer works per BYTE: FA_CHUNK bytes per workgroup, 16 per thread.
//   k_fa_summary   per chunk: does it hold a '\n', and does the line after its last one begin with '>'; the first byte of
//                  each file that is no line end (it must be a '>')
//   exclusive_scan + k_fa_compact   the carry: whether a chunk's first byte lies in a header is what the last chunk in front
//                  of it that holds a '\n' says — those chunks are compacted and each chunk looks at the one before its rank
//   k_fa_count     classes (header, line end, valid base, other) -> valid bases and header starts per chunk
//   k_fa_write     the valid bases as a DENSE stream of 2-bit codes (position: exclusive scans of the counts), one bit per
//                  dense position at which a run begins (an invalid byte or a header stands in front of it), progress marks
//   k_fa_run_count / k_fa_run_fill   the run table: where in the dense stream every run begins (its length: up to the next)
//   k_fa_run_segs / k_fa_seg_fill    the segment table: runs shorter than k dropped, long ones in pieces (fastq.cpp: kPiece)
//   k_fa_gather    one thread per output word: the 16 codes from the dense stream (overlapping pieces read codes twice)
// The result is the layout of gpu_pack_fastq word for word: tests/test_gpu_fasta_pack.py.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>

#include "device_mem.h"
#include "fasta_gpu.h"
#include "scan_gpu.h"

namespace shk {

static constexpr uint32_t FA_T = 256, FA_PER = 16;
static_assert(FA_T * FA_PER == FASTA_GPU_CHUNK, "a chunk is what one workgroup reads");
static constexpr uint64_t FA_PIECE = 16384;          // k-mers per piece of a long run (fastq.cpp: kPiece)
// one thread per item, every item (grid1 caps the grid for kernels that stride)
static inline unsigned fa_grid(uint64_t work) { const uint64_t b = (work + 255) / 256; return (unsigned)(b < 1 ? 1 : b); }
enum : uint32_t { C_END = 0, C_HDR = 1, C_VALID = 2, C_OTHER = 3 };

__device__ __forceinline__ uint32_t fa_code(uint32_t c) { return ((c >> 1) ^ (c >> 2)) & 3u; }
__device__ __forceinline__ bool fa_valid(uint32_t c) {
    const uint32_t u = (c | 0x20u) - 'a';                  // a=0 c=2 g=6 t=19
    return u < 26u && ((0x80045u >> u) & 1u);
}

// exclusive scan over the 256 threads of a workgroup (sum, or max); *total: over all of them.  Every thread calls it.
template <bool MAX> __device__ __forceinline__ uint32_t block_excl(uint32_t v, uint32_t *ws /* [4], LDS */, uint32_t *total) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    uint32_t incl = v;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = (uint32_t)__shfl_up((int)incl, o);
        if (lane >= o) incl = MAX ? (u > incl ? u : incl) : incl + u;
    }
    uint32_t excl = (uint32_t)__shfl_up((int)incl, 1);
    if (lane == 0) excl = 0;
    __syncthreads();                                       // (ws may still be read from the call before)
    if (lane == 63) ws[wid] = incl;
    __syncthreads();
    uint32_t off = 0, tot = 0;
    for (int w = 0; w < (int)(FA_T / 64); w++) {
        const uint32_t x = ws[w];
        if (w < wid) off = MAX ? (x > off ? x : off) : off + x;
        tot = MAX ? (x > tot ? x : tot) : tot + x;
    }
    if (total) *total = tot;
    return MAX ? (off > excl ? off : excl) : off + excl;
}

// the 16 bytes of a thread, the byte behind them (0 where the text ends) and whether the first one begins a line
struct FaPiece { uint8_t c[FA_PER + 1]; uint32_t len; bool at_ls; };
__device__ __forceinline__ void fa_load(const uint8_t *__restrict__ text, uint64_t n, uint64_t p0, bool vec, FaPiece &pc) {
    pc.len = p0 < n ? (uint32_t)(n - p0 < FA_PER ? n - p0 : FA_PER) : 0u;
    pc.at_ls = false;
#pragma unroll
    for (int i = 0; i <= (int)FA_PER; i++) pc.c[i] = 0;
    if (!pc.len) return;
    if (vec && pc.len == FA_PER) {
        const uint4 v = *reinterpret_cast<const uint4 *>(text + p0);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < (int)FA_PER; i++) pc.c[i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
    } else {
#pragma unroll
        for (int i = 0; i < (int)FA_PER; i++) if (i < (int)pc.len) pc.c[i] = text[p0 + i];
    }
    if (pc.len == FA_PER && p0 + FA_PER < n) pc.c[FA_PER] = text[p0 + FA_PER];
    pc.at_ls = p0 == 0 || text[p0 - 1] == '\n';
}
// what the last '\n' of the piece says about the line behind it: 0 there is none, 1 a sequence line (or the end), 2 a header
__device__ __forceinline__ uint32_t fa_last_line(const FaPiece &pc, uint64_t p0, uint64_t n) {
    uint32_t key = 0;
#pragma unroll
    for (int i = 0; i < (int)FA_PER; i++)
        if (i < (int)pc.len && pc.c[i] == '\n') key = (p0 + i + 1 < n && pc.c[i + 1] == '>') ? 2u : 1u;
    return key;
}
// the classes of the piece's bytes in order: f(i, class, begins_a_header, byte).  hdr: whether the first byte lies in a header
// line (not looked at where that byte begins a line).
template <class F> __device__ __forceinline__ void fa_walk(const FaPiece &pc, uint64_t p0, uint64_t n, bool hdr, F &&f) {
    bool at_ls = pc.at_ls;
#pragma unroll
    for (int i = 0; i < (int)FA_PER; i++) {
        if (i < (int)pc.len) {
            const uint32_t b = pc.c[i];
            const bool start = at_ls && b == '>';
            if (at_ls) hdr = start;
            const bool nl = b == '\n';
            const bool cr = b == '\r' && (p0 + i + 1 == n || pc.c[i + 1] == '\n');      // a '\r' in front of '\n', or the last byte
            const uint32_t cls = (nl || cr) ? C_END : hdr ? C_HDR : fa_valid(b) ? C_VALID : C_OTHER;
            f(i, cls, start, b);
            at_ls = nl;
        }
    }
}
// whether the thread's first byte lies in a header: from the last '\n' in front of it inside the chunk, else from the carry
__device__ __forceinline__ bool fa_state(const FaPiece &pc, uint64_t p0, uint64_t n, const uint8_t *__restrict__ text,
                                         const unsigned long long *__restrict__ nl_rank, const uint8_t *__restrict__ compact, uint32_t *ws) {
    const uint32_t key = fa_last_line(pc, p0, n);
    const uint32_t before = block_excl<true>(key ? ((threadIdx.x + 1u) << 2) | key : 0u, ws, nullptr) & 3u;
    if (before) return before == 2u;
    const unsigned long long r = nl_rank[blockIdx.x];      // chunks in front of this one that hold a '\n'
    return r ? compact[r - 1] == 2u : text[0] == '>';      // (none: the line began with the text)
}

// ---- the carry ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FA_T) void k_fa_summary(const uint8_t *__restrict__ text, uint64_t n, uint64_t off2, bool vec,
                                                     unsigned long long *__restrict__ nl_flag, uint8_t *__restrict__ last_line,
                                                     unsigned long long *__restrict__ first_byte /* [2]: min of pos << 8 | byte, per file */) {
    __shared__ uint32_t ws[4];
    __shared__ unsigned long long wmin[2][4];
    const uint64_t p0 = (uint64_t)blockIdx.x * FASTA_GPU_CHUNK + (uint64_t)threadIdx.x * FA_PER;
    FaPiece pc;
    fa_load(text, n, p0, vec, pc);
    const uint32_t key = fa_last_line(pc, p0, n);
    uint32_t top = 0;
    (void)block_excl<true>(key ? ((threadIdx.x + 1u) << 2) | key : 0u, ws, &top);
    if (threadIdx.x == 0) { nl_flag[blockIdx.x] = top ? 1ull : 0ull; last_line[blockIdx.x] = (uint8_t)(top & 3u); }
    // the first byte that is no line end (the class C_END does not depend on the header state)
    unsigned long long m[2] = {~0ull, ~0ull};
    fa_walk(pc, p0, n, false, [&](int i, uint32_t cls, bool, uint32_t b) {
        const uint64_t p = p0 + (uint64_t)i;
        const int f = p >= off2 ? 1 : 0;
        if (cls != C_END && m[f] == ~0ull) m[f] = (p << 8) | b;
    });
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    for (int f = 0; f < 2; f++) {
        unsigned long long v = m[f];
        for (int o = 32; o > 0; o >>= 1) { const unsigned long long u = __shfl_down(v, o); if (u < v) v = u; }
        if (lane == 0) wmin[f][wid] = v;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const int f = threadIdx.x;
        unsigned long long v = wmin[f][0];
        for (int w = 1; w < 4; w++) if (wmin[f][w] < v) v = wmin[f][w];
        // (nearly every chunk has such a byte and only the first one counts: look before asking for the atomic)
        if (v != ~0ull && v < *(volatile unsigned long long *)&first_byte[f]) atomicMin(&first_byte[f], v);
    }
}
__global__ __launch_bounds__(256) void k_fa_compact(const unsigned long long *__restrict__ nl_rank, const uint8_t *__restrict__ last_line,
                                                    uint64_t n_chunks, uint8_t *__restrict__ compact) {
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c < n_chunks && last_line[c]) compact[nl_rank[c]] = last_line[c];
}

// ---- counts ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FA_T) void k_fa_count(const uint8_t *__restrict__ text, uint64_t n, bool vec,
                                                   const unsigned long long *__restrict__ nl_rank, const uint8_t *__restrict__ compact,
                                                   unsigned long long *__restrict__ cnt_valid, unsigned long long *__restrict__ cnt_hdr,
                                                   unsigned long long *__restrict__ input_bases /* [64] partial sums */) {
    __shared__ uint32_t ws[4];
    const uint64_t p0 = (uint64_t)blockIdx.x * FASTA_GPU_CHUNK + (uint64_t)threadIdx.x * FA_PER;
    FaPiece pc;
    fa_load(text, n, p0, vec, pc);
    const bool hdr = fa_state(pc, p0, n, text, nl_rank, compact, ws);
    uint32_t nv = 0, nh = 0, ni = 0;
    fa_walk(pc, p0, n, hdr, [&](int, uint32_t cls, bool start, uint32_t) {
        nv += cls == C_VALID; nh += start; ni += cls == C_VALID || cls == C_OTHER;
    });
    uint32_t tv = 0, th = 0, ti = 0;
    (void)block_excl<false>(nv, ws, &tv);
    (void)block_excl<false>(nh, ws, &th);
    (void)block_excl<false>(ni, ws, &ti);
    if (threadIdx.x == 0) {
        cnt_valid[blockIdx.x] = tv; cnt_hdr[blockIdx.x] = th;
        if (ti) atomicAdd(&input_bases[blockIdx.x & 63u], (unsigned long long)ti);
    }
}

// ---- the dense stream, the run starts, the progress marks ----------------------------------------------------------------
struct FaMarks {
    unsigned long long *marks; uint64_t every, read_base, first_mark, n_marks;
    uint64_t off2, part1_len, first2;          // first2: where the first header of file 2 begins (it ends the last record of file 1)
};
__global__ __launch_bounds__(FA_T) void k_fa_write(const uint8_t *__restrict__ text, uint64_t n, bool vec,
                                                   const unsigned long long *__restrict__ nl_rank, const uint8_t *__restrict__ compact,
                                                   const unsigned long long *__restrict__ valid_off, const unsigned long long *__restrict__ hdr_off,
                                                   uint64_t n_valid, uint32_t *__restrict__ dense, uint32_t *__restrict__ run_bits, FaMarks fm) {
    __shared__ uint32_t ws[4];
    const uint64_t p0 = (uint64_t)blockIdx.x * FASTA_GPU_CHUNK + (uint64_t)threadIdx.x * FA_PER;
    FaPiece pc;
    fa_load(text, n, p0, vec, pc);
    const bool hdr = fa_state(pc, p0, n, text, nl_rank, compact, ws);
    uint32_t nv = 0, nh = 0;
    fa_walk(pc, p0, n, hdr, [&](int, uint32_t cls, bool start, uint32_t) { nv += cls == C_VALID; nh += start; });
    uint64_t d = valid_off[blockIdx.x] + block_excl<false>(nv, ws, nullptr);        // dense position of the thread's next valid base
    uint64_t g = hdr_off[blockIdx.x] + block_excl<false>(nh, ws, nullptr);          // index of the thread's next header
    uint64_t marked = ~0ull;                               // the dense position whose run bit this thread set last
    uint64_t wi = d >> 4; uint32_t word = 0;               // the dense word in hand
    auto put_word = [&]() {
        if (word) atomicOr(&dense[wi], word);              // (a word is shared with the neighbouring threads)
        word = 0;
    };
    if (blockIdx.x == 0 && threadIdx.x == 0 && n_valid) atomicOr(&run_bits[0], 1u);
    fa_walk(pc, p0, n, hdr, [&](int i, uint32_t cls, bool start, uint32_t b) {
        if (cls == C_VALID) {
            if ((d >> 4) != wi) { put_word(); wi = d >> 4; }
            word |= fa_code(b) << (2u * ((uint32_t)d & 15u));
            d++;
        } else if (cls == C_OTHER || start) {
            // whatever valid base comes next begins a run (d == n_valid: none does)
            if (d != marked && d < n_valid) { atomicOr(&run_bits[d >> 5], 1u << ((uint32_t)d & 31u)); marked = d; }
        }
        if (start) {
            // this header ends record g - 1: a mark where the number of records read is a multiple of `every`
            const uint64_t done = fm.read_base + g;
            if (fm.every && g && done % fm.every == 0) {
                const uint64_t j = done / fm.every - 1 - fm.first_mark, p = p0 + (uint64_t)i;
                if (j < fm.n_marks) fm.marks[j] = p < fm.off2 ? p : (p == fm.first2 ? fm.part1_len : ((p - fm.off2) | (1ull << 63)));
            }
            g++;
        }
    });
    put_word();
}

// ---- the run table ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_fa_run_count(const uint32_t *__restrict__ run_bits, uint64_t n_words, unsigned long long *__restrict__ cnt) {
    const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w < n_words) cnt[w] = (unsigned long long)__popc(run_bits[w]);
}
__global__ __launch_bounds__(256) void k_fa_run_fill(const uint32_t *__restrict__ run_bits, uint64_t n_words, const unsigned long long *__restrict__ rank,
                                                     uint64_t n_runs, uint64_t n_valid, unsigned long long *__restrict__ run_pos /* [n_runs + 1] */) {
    const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w == 0) run_pos[n_runs] = n_valid;
    if (w >= n_words) return;
    uint32_t m = run_bits[w];
    unsigned long long o = rank[w];
    while (m) {
        const uint32_t bit = (uint32_t)__ffs((int)m) - 1u;
        if (o < n_runs) run_pos[o] = (w << 5) + bit;
        o++;
        m &= m - 1u;
    }
}
// segments and packed bases of a run of L bases: none below k, else ceil((L - k + 1) / FA_PIECE) pieces that overlap by k - 1
__device__ __forceinline__ uint64_t fa_pieces(uint64_t L, uint32_t k) { return L < k ? 0 : (L - k + 1 + FA_PIECE - 1) / FA_PIECE; }
__global__ __launch_bounds__(256) void k_fa_run_segs(const unsigned long long *__restrict__ run_pos, uint64_t n_runs, uint32_t k,
                                                     unsigned long long *__restrict__ seg_cnt, unsigned long long *__restrict__ base_cnt) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_runs) return;
    const uint64_t L = run_pos[j + 1] - run_pos[j], m = fa_pieces(L, k);
    seg_cnt[j] = m;
    base_cnt[j] = m ? L + (m - 1) * (uint64_t)(k - 1) : 0;
}
__global__ __launch_bounds__(256) void k_fa_seg_fill(const unsigned long long *__restrict__ run_pos, uint64_t n_runs, uint32_t k,
                                                     const unsigned long long *__restrict__ seg_first, const unsigned long long *__restrict__ base_first,
                                                     uint64_t n_seg, uint64_t n_bases, uint32_t *__restrict__ seg_off /* [n_seg + 1] */,
                                                     unsigned long long *__restrict__ seg_src /* [n_seg] */) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j == 0) seg_off[n_seg] = (uint32_t)n_bases;
    if (j >= n_runs) return;
    const uint64_t a = run_pos[j], L = run_pos[j + 1] - a, m = fa_pieces(L, k);
    const uint64_t s0 = seg_first[j], b0 = base_first[j];
    for (uint64_t i = 0; i < m && s0 + i < n_seg; i++) {
        seg_off[s0 + i] = (uint32_t)(b0 + i * (FA_PIECE + k - 1));
        seg_src[s0 + i] = a + i * FA_PIECE;
    }
}

// ---- gather-pack -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_fa_gather(const uint32_t *__restrict__ dense /* two words readable behind the last code */,
                                                   const uint32_t *__restrict__ seg_off, const unsigned long long *__restrict__ seg_src,
                                                   uint64_t n_seg, uint64_t n_bases, uint32_t *__restrict__ out, uint64_t n_words) {
    const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n_words) return;
    const uint64_t pos0 = w << 4;
    uint32_t word = 0;
    if (pos0 < n_bases && n_seg) {
        uint64_t lo = 0, hi = n_seg - 1;                   // the last segment that begins at or in front of pos0
        while (lo < hi) {
            const uint64_t mid = (lo + hi + 1) >> 1;
            if ((uint64_t)seg_off[mid] <= pos0) lo = mid; else hi = mid - 1;
        }
        uint64_t s = lo, pos = pos0;
        const uint64_t end = pos0 + 16 < n_bases ? pos0 + 16 : n_bases;
        while (pos < end && s < n_seg) {
            const uint64_t se = seg_off[s + 1], b = end < se ? end : se;
            const uint32_t len = (uint32_t)(b - pos);
            const uint64_t q = seg_src[s] + (pos - (uint64_t)seg_off[s]);
            const uint64_t two = (uint64_t)dense[q >> 4] | ((uint64_t)dense[(q >> 4) + 1] << 32);
            const uint64_t bits = (two >> (2u * ((uint32_t)q & 15u))) & ((1ull << (2u * len)) - 1ull);
            word |= (uint32_t)(bits << (2u * (uint32_t)(pos - pos0)));
            pos = b;
            if (pos == se) s++;
        }
    }
    out[w] = word;
}

// ---- the host side ---------------------------------------------------------------------------------------------------------
int gpu_pack_fasta(const uint8_t *t1, size_t n1, const uint8_t *t2, size_t n2, uint32_t k, uint64_t every, void *stream_v,
                   GpuPacked &out, std::string &err, uint64_t read_base, const GpuText *uploaded) {
    hipStream_t st = (hipStream_t)stream_v;
    out = GpuPacked();
    PoolScope sc(st, "FASTA packer");
    if (uploaded && t2) { err = "an uploaded text cannot be combined with a second file"; return -1; }
    if (k < 2) { err = "k too small"; return -1; }
    const size_t e1 = uploaded ? uploaded->e : n1, e2 = t2 ? n2 : 0;
    const bool unterm1 = !uploaded && e1 && t1[e1 - 1] != '\n';
    const size_t off2 = e1 + ((unterm1 && e2) ? 1 : 0);      // (a newline is supplied between the files)
    const size_t n = off2 + e2;
    auto empty_batch = [&](uint64_t n_reads, uint64_t n_input) -> int {
        uint32_t *so = sc.get<uint32_t>(2, err), *bs = sc.get<uint32_t>(2, err);
        if (!so || !bs) return -4;
        HIPCHK(hipMemsetAsync(so, 0, 8, st)); HIPCHK(hipMemsetAsync(bs, 0, 8, st));
        HIPCHK(hipStreamSynchronize(st));
        out.bases_bytes = sc.keep(bs); out.seg_off_bytes = sc.keep(so);
        out.d_bases = bs; out.d_seg_off = so; out.n_reads = n_reads; out.n_input_bases = n_input;
        return 0;
    };
    if (n == 0) return empty_batch(0, 0);
    uint8_t *text = uploaded ? uploaded->d : sc.get<uint8_t>(n + 32, err);
    if (!text) return -4;
    const bool vec = ((uintptr_t)text & 15u) == 0;
    // (the guard exists before the first event does: whatever was created is destroyed on every way out)
    struct Events { hipEvent_t e[3] = {nullptr, nullptr, nullptr}; ~Events() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); } } evs;
    for (hipEvent_t &x : evs.e) HIPCHK(hipEventCreate(&x));
    const hipEvent_t ev0 = evs.e[0], ev1 = evs.e[1], ev2 = evs.e[2];
    // upload and kernels of this text, on every way out that packed it (a text that keeps nothing ran the kernels too)
    auto stamp = [&]() -> int {
        HIPCHK(hipEventRecord(ev2, st));
        HIPCHK(hipStreamSynchronize(st));
        float a = 0, b = 0;
        (void)hipEventElapsedTime(&a, ev0, ev1); (void)hipEventElapsedTime(&b, ev1, ev2);
        out.h2d_ms = uploaded ? uploaded->h2d_ms : a; out.kernels_ms = b;
        return 0;
    };
    HIPCHK(hipEventRecord(ev0, st));
    if (!uploaded) {
        if (e1) HIPCHK(hipMemcpyAsync(text, t1, e1, hipMemcpyHostToDevice, st));
        if (off2 > e1) HIPCHK(hipMemsetAsync(text + e1, '\n', 1, st));
        if (e2) HIPCHK(hipMemcpyAsync(text + off2, t2, e2, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemsetAsync(text + n, 0, 32, st));
    }
    HIPCHK(hipEventRecord(ev1, st));

    // ---- the carry and the counts
    const uint64_t n_chunks = (n + FASTA_GPU_CHUNK - 1) / FASTA_GPU_CHUNK;
    unsigned long long *nl_rank = sc.get<unsigned long long>(n_chunks, err);
    unsigned long long *cnt_valid = sc.get<unsigned long long>(n_chunks, err), *cnt_hdr = sc.get<unsigned long long>(n_chunks, err);
    uint8_t *last_line = sc.get<uint8_t>(n_chunks, err), *compact = sc.get<uint8_t>(n_chunks, err);
    // d_tot: [0] chunks with a '\n' [1] valid bases [2] headers [3] runs [4] segments [5] packed bases [6] [7] the first byte
    // of file 1 / 2 that is no line end [16..80) input bases, partial sums
    unsigned long long *d_tot = sc.get<unsigned long long>(16 + 64, err);
    if (!nl_rank || !cnt_valid || !cnt_hdr || !last_line || !compact || !d_tot) return -4;
    HIPCHK(hipMemsetAsync(d_tot, 0, (16 + 64) * 8, st));
    HIPCHK(hipMemsetAsync(d_tot + 6, 0xFF, 16, st));
    hipLaunchKernelGGL(k_fa_summary, dim3((unsigned)n_chunks), dim3(FA_T), 0, st, text, (uint64_t)n, (uint64_t)off2, vec, nl_rank, last_line, d_tot + 6);
    if (int rc = exclusive_scan(nl_rank, n_chunks, d_tot + 0, st, sc, err)) return rc;
    hipLaunchKernelGGL(k_fa_compact, dim3(fa_grid(n_chunks)), dim3(256), 0, st, nl_rank, last_line, n_chunks, compact);
    hipLaunchKernelGGL(k_fa_count, dim3((unsigned)n_chunks), dim3(FA_T), 0, st, text, (uint64_t)n, vec, nl_rank, compact, cnt_valid, cnt_hdr, d_tot + 16);
    if (int rc = exclusive_scan(cnt_valid, n_chunks, d_tot + 1, st, sc, err)) return rc;
    if (int rc = exclusive_scan(cnt_hdr, n_chunks, d_tot + 2, st, sc, err)) return rc;
    HIPCHK(hipGetLastError());
    unsigned long long h[16 + 64];
    HIPCHK(hipMemcpyAsync(h, d_tot, sizeof h, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    // the first line of a file that is not blank must be a header: the host packer words the message
    for (int f = 0; f < 2; f++) if (h[6 + f] != ~0ull && (h[6 + f] & 0xFFu) != '>') return 1;
    const uint64_t n_valid = h[1], n_reads = h[2];
    uint64_t n_input = 0;
    for (int i = 0; i < 64; i++) n_input += h[16 + i];

    // ---- progress marks: one where the records read reach a multiple of `every`; the last record ends with the text
    unsigned long long *marks = nullptr;
    uint64_t n_marks = 0, first_mark = 0;
    const unsigned long long end_mark = e2 ? ((unsigned long long)e2 | (1ull << 63)) : (unsigned long long)e1;
    if (every) {
        first_mark = read_base / every;
        n_marks = (read_base + n_reads) / every - first_mark;
        out.first_mark = first_mark;
        if (n_marks) {
            marks = sc.get<unsigned long long>(n_marks, err);
            if (!marks) return -4;
            if ((read_base + n_reads) % every == 0) HIPCHK(hipMemcpyAsync(marks + (n_marks - 1), &end_mark, 8, hipMemcpyHostToDevice, st));
        }
    }
    auto finish_marks = [&]() -> int {
        if (n_marks) {
            out.progress_bytes.resize(n_marks);
            HIPCHK(hipMemcpyAsync(out.progress_bytes.data(), marks, n_marks * 8, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
        }
        return 0;
    };
    const FaMarks fm{marks, every, read_base, first_mark, n_marks, (uint64_t)off2, (uint64_t)e1, h[7] == ~0ull ? ~0ull : (uint64_t)(h[7] >> 8)};

    // ---- the dense stream and the run bits
    const uint64_t dense_words = (n_valid >> 4) + 3, bit_words = (n_valid >> 5) + 1;
    uint32_t *dense = sc.get<uint32_t>(dense_words, err), *run_bits = sc.get<uint32_t>(bit_words, err);
    unsigned long long *run_cnt = sc.get<unsigned long long>(bit_words, err);
    if (!dense || !run_bits || !run_cnt) return -4;
    HIPCHK(hipMemsetAsync(dense, 0, dense_words * 4, st));
    HIPCHK(hipMemsetAsync(run_bits, 0, bit_words * 4, st));
    hipLaunchKernelGGL(k_fa_write, dim3((unsigned)n_chunks), dim3(FA_T), 0, st, text, (uint64_t)n, vec, nl_rank, compact, cnt_valid, cnt_hdr,
                       n_valid, dense, run_bits, fm);
    HIPCHK(hipGetLastError());
    if (n_valid == 0) {
        if (int rc = finish_marks()) return rc;
        if (int rc = stamp()) return rc;
        return empty_batch(n_reads, n_input);
    }
    // ---- the run table
    hipLaunchKernelGGL(k_fa_run_count, dim3(fa_grid(bit_words)), dim3(256), 0, st, run_bits, bit_words, run_cnt);
    if (int rc = exclusive_scan(run_cnt, bit_words, d_tot + 3, st, sc, err)) return rc;
    unsigned long long n_runs = 0;
    HIPCHK(hipMemcpyAsync(&n_runs, d_tot + 3, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    unsigned long long *run_pos = sc.get<unsigned long long>(n_runs + 1, err);
    unsigned long long *seg_cnt = sc.get<unsigned long long>(n_runs, err), *base_cnt = sc.get<unsigned long long>(n_runs, err);
    if (!run_pos || !seg_cnt || !base_cnt) return -4;
    hipLaunchKernelGGL(k_fa_run_fill, dim3(fa_grid(bit_words)), dim3(256), 0, st, run_bits, bit_words, run_cnt, (uint64_t)n_runs, n_valid, run_pos);
    // ---- the segment table
    hipLaunchKernelGGL(k_fa_run_segs, dim3(fa_grid(n_runs)), dim3(256), 0, st, run_pos, (uint64_t)n_runs, k, seg_cnt, base_cnt);
    if (int rc = exclusive_scan(seg_cnt, n_runs, d_tot + 4, st, sc, err)) return rc;
    if (int rc = exclusive_scan(base_cnt, n_runs, d_tot + 5, st, sc, err)) return rc;
    HIPCHK(hipGetLastError());
    unsigned long long h2[2];
    HIPCHK(hipMemcpyAsync(h2, d_tot + 4, sizeof h2, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const uint64_t n_seg = h2[0], n_bases = h2[1];
    if (n_bases >= 0xFFFFFFF0ull) return 1;               // more than a batch holds: the host packer says so
    if (n_seg == 0) {
        if (int rc = finish_marks()) return rc;
        if (int rc = stamp()) return rc;
        return empty_batch(n_reads, n_input);
    }
    const uint64_t n_words = (n_bases >> 4) + 2;          // partial word + one spare word (as PackedReads::finish)
    uint32_t *seg_off = sc.get<uint32_t>(n_seg + 1, err), *bases = sc.get<uint32_t>(n_words, err);
    unsigned long long *seg_src = sc.get<unsigned long long>(n_seg, err);
    if (!seg_off || !bases || !seg_src) return -4;
    hipLaunchKernelGGL(k_fa_seg_fill, dim3(fa_grid(n_runs)), dim3(256), 0, st, run_pos, (uint64_t)n_runs, k, seg_cnt, base_cnt, n_seg, n_bases, seg_off, seg_src);
    hipLaunchKernelGGL(k_fa_gather, dim3(fa_grid(n_words)), dim3(256), 0, st, dense, seg_off, seg_src, n_seg, n_bases, bases, n_words);
    HIPCHK(hipGetLastError());
    if (int rc = finish_marks()) return rc;
    if (int rc = stamp()) return rc;
    out.bases_bytes = sc.keep(bases); out.seg_off_bytes = sc.keep(seg_off);
    out.d_bases = bases; out.d_seg_off = seg_off;
    out.n_seg = n_seg; out.n_bases = n_bases; out.n_reads = n_reads; out.n_input_bases = n_input;
    return 0;
}

}  // namespace shk
