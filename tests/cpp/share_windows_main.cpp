// The host planning of a rank's windows (csrc/share_windows.h) as a stand-alone program: hand-made ISIZE lists and seeded
// random ones through plan_share_windows, against the composition of plan_fastq_slices and plan_bgzf_windows and against the
// properties the windows must have.  Built with AddressSanitizer and UBSan by tests/test_share_windows_host.py.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "share_windows.h"

using namespace shk;

static int n_checked = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); exit(1); } n_checked++; } while (0)

static void check_list(const std::vector<uint32_t> &isize, uint32_t world, uint64_t budget) {
    const size_t B = isize.size();
    std::vector<uint64_t> run;
    plan_fastq_slices(isize.data(), B, world, run);
    std::vector<int> covered(B, 0);
    for (uint32_t r = 0; r < world; r++) {
        std::vector<uint64_t> first; uint64_t end = 0;
        const int rc = plan_share_windows(isize.data(), B, world, r, budget, first, end);
        const size_t b0 = (size_t)run[r], b1 = (size_t)run[r + 1];
        std::vector<uint64_t> want;
        const int rc2 = plan_bgzf_windows(isize.data() + b0, b1 - b0, budget, want);
        CHECK((rc == 0) == (rc2 == 0));
        if (rc) { CHECK(rc == -1 && first.empty()); for (size_t b = b0; b < b1; b++) covered[b]++; continue; }
        CHECK(end == b1 && first.size() == want.size());
        for (size_t w = 0; w < first.size(); w++) CHECK(first[w] == want[w] + b0);
        uint64_t run_text = 0;
        for (size_t b = b0; b < b1; b++) run_text += isize[b];
        CHECK(first.empty() == (b0 == b1));
        if (!first.empty()) CHECK(first[0] == b0);
        for (size_t w = 0; w < first.size(); w++) {
            const size_t wb0 = (size_t)first[w], wb1 = w + 1 < first.size() ? (size_t)first[w + 1] : b1;
            CHECK(wb0 < wb1 && wb1 <= b1);                  // consecutive, none without a block
            uint64_t text = 0;
            for (size_t b = wb0; b < wb1; b++) { text += isize[b]; covered[b]++; }
            CHECK(text <= budget);
            CHECK(text > 0 || run_text == 0);
        }
    }
    for (size_t b = 0; b < B; b++) CHECK(covered[b] == 1);  // over all ranks every block lies in one window
}

int main() {
    // by hand: no blocks, one block, empty blocks anywhere, more ranks than blocks, a block equal to the budget
    check_list({}, 1, 65536);
    check_list({}, 3, 65536);
    check_list({4096}, 1, 65536);
    check_list({4096}, 4, 4096);
    check_list({0, 0, 0}, 2, 65536);
    check_list({0, 100, 0, 0, 200, 0, 300, 0}, 3, 300);
    check_list({65536, 65536, 65536, 65536, 0}, 2, 65536);
    check_list({10, 20, 30}, 7, 30);
    {
        // a block beyond the budget fails for the rank that holds it, and for that rank alone
        const std::vector<uint32_t> isize = {100, 100, 5000, 100};
        std::vector<uint64_t> first; uint64_t end = 0;
        CHECK(plan_share_windows(isize.data(), isize.size(), 1, 0, 4999, first, end) == -1 && first.empty());
        CHECK(plan_share_windows(isize.data(), isize.size(), 1, 0, 5000, first, end) == 0 && first.size() == 3 && first[1] == 2 && first[2] == 3);
        CHECK(plan_share_windows(isize.data(), isize.size(), 2, 2, 5000, first, end) == -2);
        CHECK(plan_share_windows(isize.data(), isize.size(), 0, 0, 5000, first, end) == -2);
        check_list(isize, 3, 4999);
    }
    // seeded random lists (a linear congruential generator: the same everywhere)
    uint64_t s = 0x9E3779B97F4A7C15ull;
    auto rnd = [&s](uint64_t n) { s = s * 6364136223846793005ull + 1442695040888963407ull; return (s >> 33) % n; };
    for (int it = 0; it < 200; it++) {
        std::vector<uint32_t> isize(rnd(120));
        for (uint32_t &v : isize) v = rnd(5) == 0 ? 0u : (uint32_t)rnd(65537);
        check_list(isize, 1 + (uint32_t)rnd(9), 65536 + rnd(400000));
    }
    printf("ok: %d checks\n", n_checked);
    return 0;
}
