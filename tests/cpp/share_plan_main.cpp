// The host planning of the share readers (csrc/share_plan.h) as a stand-alone program: for every line of a case list it plans
// one rank's share of the files named there and prints the plan; tests/test_share_plan_host.py writes the files and the list
// and compares the plans with its own computation.  Host sources only (fastq.cpp, inflate_mt.cpp, zlib); built with
// AddressSanitizer and UBSan.
//   a line:  FMT RANK WORLD MIN BATCH FILE1 FILE2
//   FMT fastq | fasta;  MIN / BATCH: SHK_GUNZIP_DEVICE_MIN / SHK_BATCH_BASES for this case, "-" = unset;
//   FILE: a path, "-" = no file (null, 0), "null:N" = a null pointer with a size of N
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <fstream>
#include <sstream>
#include <string>

#include "share_plan.h"

using namespace shk;

// the file in a block of exactly its size (a read past its end is the sanitizer's)
struct Bytes { uint8_t *p = nullptr; size_t n = 0; ~Bytes() { free(p); } };
static void load(const std::string &arg, Bytes &b) {
    if (arg == "-") return;
    if (arg.rfind("null:", 0) == 0) { b.n = (size_t)strtoull(arg.c_str() + 5, nullptr, 10); return; }
    FILE *f = fopen(arg.c_str(), "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", arg.c_str()); exit(2); }
    fseek(f, 0, SEEK_END); b.n = (size_t)ftell(f); fseek(f, 0, SEEK_SET);
    b.p = (uint8_t *)malloc(b.n ? b.n : 1);
    if (fread(b.p, 1, b.n, f) != b.n) { fprintf(stderr, "cannot read %s\n", arg.c_str()); exit(2); }
    fclose(f);
}
static void env(const char *name, const std::string &v) { if (v == "-") unsetenv(name); else setenv(name, v.c_str(), 1); }

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: share_plan_main CASES\n"); return 2; }
    std::ifstream in(argv[1]);
    std::string line;
    int n_cases = 0;
    for (int c = 0; std::getline(in, line); c++) {
        std::istringstream ls(line);
        std::string fmt, min_s, batch_s, a1, a2; uint32_t rank = 0, world = 0;
        if (!(ls >> fmt >> rank >> world >> min_s >> batch_s >> a1 >> a2)) { fprintf(stderr, "bad line %d\n", c); return 2; }
        env("SHK_GUNZIP_DEVICE_MIN", min_s); env("SHK_BATCH_BASES", batch_s);
        Bytes f1, f2;
        load(a1, f1); load(a2, f2);
        SharePlan pl;
        std::string err;
        const int plan_rc = plan_share(fmt == "fasta" ? RecFmt::Fasta : RecFmt::Fastq, f1.p, f1.n, f2.p, f2.n, rank, world, pl, err);
        const int est_rc = plan_rc ? 0 : estimate_share(pl, err);
        const Knobs kn;
        printf("case %d plan_rc=%d est_rc=%d nf=%d total=%llu in_batches=%d batch_bases=%llu err=%s\n", c, plan_rc, est_rc, plan_rc ? 0 : pl.nf,
               (unsigned long long)pl.total, (int)(!plan_rc && !est_rc && share_in_batches(pl.sf, pl.total, kn)), (unsigned long long)kn.batch_bases, err.c_str());
        for (int i = 0; !plan_rc && i < pl.nf; i++) {
            const ShareFile &F = pl.f[i];
            printf("file %d %d gz=%d walked=%d blocks=%zu text=%llu c0=%llu c1=%llu host=%d l=%zu e=%zu s0=%llu s1=%llu end=%llu est=%llu\n", c, i, (int)F.gz, (int)F.walked,
                   F.chain.blocks.size(), (unsigned long long)F.chain.text, (unsigned long long)F.c0, (unsigned long long)F.c1, (int)F.host_text, F.l, F.e,
                   (unsigned long long)F.s0, (unsigned long long)F.s1, (unsigned long long)(F.host_text ? F.slice_end() : 0), (unsigned long long)F.est);
        }
        n_cases++;
    }
    printf("ok: %d cases\n", n_cases);
    return 0;
}
