// share_windows.h — the host planning of how FASTQ files are cut among ranks and into windows: plain arithmetic on the ISIZE
// fields of a BGZF chain (what the host knows of a file before a byte crosses PCIe).  No HIP and no zlib in here: a host
// compiler takes this header alone (tests/cpp/share_windows_main.cpp runs it under AddressSanitizer and UBSan).
//     plan_fastq_slices   the ranks' runs of blocks (the sharded FASTQ entry point, fastq.h: the slice rule)
//     plan_bgzf_windows   a run of blocks in windows of at most `budget` bytes of text (inflate_gpu.h: BgzfWindows)
//     plan_share_windows  the two together: the windows of ONE rank's run (inflate_gpu.h: BgzfShareWindows)
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

namespace shk {

// the record format by which a slice, a window or a piece is cut: 4-line FASTQ, or FASTA (fastq.h states both rules)
enum class RecFmt { Fastq, Fasta };

// the nominal cut c_r of a text of e bytes among `world` ranks
inline uint64_t slice_cut(uint64_t e, uint32_t r, uint32_t world) { return (uint64_t)((unsigned __int128)e * r / world); }

// The windows of a BGZF chain (preprocess.cpp, route 2): runs of consecutive blocks whose text (the sum of their ISIZE
// fields) is at most `budget` bytes.  first[w] = the first block of window w; window w ends where window w + 1 begins, the
// last one at n_blocks.  Every block lies in exactly one window and no window is without text, unless the file has none
// (then there is one window, or none for a file of no blocks).  Empty blocks ride with the window in front of them.
// Returns 0, or -1 when a block alone exceeds the budget.
inline int plan_bgzf_windows(const uint32_t *isize, size_t n_blocks, uint64_t budget, std::vector<uint64_t> &first) {
    first.clear();
    uint64_t sum = 0;
    for (size_t i = 0; i < n_blocks; i++) {
        if (isize[i] > budget) return -1;
        if (first.empty() || sum + isize[i] > budget) { first.push_back(i); sum = 0; }      // (an empty block never opens a window but the first)
        sum += isize[i];
    }
    return 0;
}

// The runs of a BGZF chain that the ranks of the sharded FASTQ entry point inflate: world runs of consecutive blocks,
// first[r] = the first block whose text offset (the sum of the ISIZE fields in front of it) is >= r * text / world, first[0]
// = 0, first[world] = n_blocks.  Empty blocks may sit anywhere; more ranks than blocks gives empty runs.
inline void plan_fastq_slices(const uint32_t *isize, size_t n_blocks, uint32_t world, std::vector<uint64_t> &first) {
    uint64_t text = 0;
    for (size_t i = 0; i < n_blocks; i++) text += isize[i];
    first.assign((size_t)world + 1, n_blocks);
    size_t b = 0; uint64_t off = 0;                       // off: the text offset of block b
    for (uint32_t r = 0; r < world; r++) {
        const uint64_t want = r ? slice_cut(text, r, world) : 0;
        while (b < n_blocks && off < want) off += isize[b++];
        first[r] = b;
    }
}

// The windows of rank `rank`'s run: plan_fastq_slices, then plan_bgzf_windows on the run's blocks alone.  first[w] = the
// first block of window w, counted in the FILE; the last window ends where the run ends, run_end.  An empty run has no
// window.  Returns 0, -1 when a block of the run alone exceeds the budget, -2 for a rank beyond the world.
inline int plan_share_windows(const uint32_t *isize, size_t n_blocks, uint32_t world, uint32_t rank, uint64_t budget,
                              std::vector<uint64_t> &first, uint64_t &run_end) {
    first.clear(); run_end = 0;
    if (world == 0 || rank >= world) return -2;
    std::vector<uint64_t> run;
    plan_fastq_slices(isize, n_blocks, world, run);
    const size_t b0 = (size_t)run[rank], b1 = (size_t)run[rank + 1];
    run_end = b1;
    if (plan_bgzf_windows(isize + b0, b1 - b0, budget, first)) { first.clear(); return -1; }
    for (uint64_t &f : first) f += b0;
    return 0;
}

}  // namespace shk
