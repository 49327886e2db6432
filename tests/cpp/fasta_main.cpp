// fasta_main.cpp — the host FASTA packer (csrc/fastq.cpp: pack_fasta) as a stand-alone program, for a build with
// AddressSanitizer and UBSan (tests/test_fasta_host.py).  Usage: fasta_main <k> <file>...
// Every file is packed twice: plainly, and with a progress mark after every record and a batch handed over every second
// record (finish + reset_stream, as the library's flush does); both ways must agree.  One line per file:
//   <rc> <n_seg> <n_bases> <n_reads> <n_input_bases> <checksum of seg_off and the words>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <vector>

#include "fastq.h"

using namespace shk;

static uint64_t mix(uint64_t h, uint64_t v) { h ^= v + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2); return h; }

int main(int argc, char **argv) {
    if (argc < 3) { fprintf(stderr, "usage: fasta_main <k> <file>...\n"); return 2; }
    const uint32_t k = (uint32_t)atoi(argv[1]);
    for (int a = 2; a < argc; a++) {
        FILE *f = fopen(argv[a], "rb");
        if (!f) { fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
        std::vector<uint8_t> text;
        uint8_t buf[65536];
        for (size_t got; (got = fread(buf, 1, sizeof buf, f)) > 0;) text.insert(text.end(), buf, buf + got);
        fclose(f);
        // (an exact-size heap copy: a read one byte past the text is a finding)
        uint8_t *exact = (uint8_t *)malloc(text.size() ? text.size() : 1);
        if (!exact) return 2;
        for (size_t i = 0; i < text.size(); i++) exact[i] = text[i];
        PackedReads pr; std::string err;
        const int rc = pack_fasta(exact, text.size(), k, pr, err);
        uint64_t sum = 0;
        if (!rc) {
            pr.finish();
            if (pr.bases.size() != (size_t)(pr.n_bases >> 4) + 2 || pr.seg_off.back() != pr.n_bases) { fprintf(stderr, "%s: layout\n", argv[a]); return 1; }
            for (uint32_t v : pr.seg_off) sum = mix(sum, v);
            for (uint32_t v : pr.bases) sum = mix(sum, v);
        } else if (rc != -3 || err.find("FASTA") == std::string::npos) { fprintf(stderr, "%s: rc %d %s\n", argv[a], rc, err.c_str()); return 1; }
        // the same text with progress and flush
        PackedReads pb; std::string err2;
        uint64_t marks = 0, last_bytes = 0, flushed_bases = 0;
        bool order_ok = true;
        auto prog = [&](uint64_t reads, uint64_t bytes, uint64_t total) { marks++; order_ok = order_ok && reads == marks && bytes >= last_bytes && bytes <= total; last_bytes = bytes; };
        auto flush = [&](PackedReads &p) -> int { p.finish(); flushed_bases += p.n_bases; p.reset_stream(); return 0; };
        const int rc2 = pack_fasta(exact, text.size(), k, pb, err2, 1, prog, 2, 0, flush, 7);
        if (!rc2) { pb.finish(); flushed_bases += pb.n_bases; }
        if (rc2 != rc || !order_ok || (!rc && (marks != pr.n_reads || pb.n_reads != pr.n_reads || flushed_bases != pr.n_bases || pb.n_input_bases != pr.n_input_bases))) {
            fprintf(stderr, "%s: the flushing run differs (rc %d / %d, marks %llu, reads %llu / %llu, bases %llu / %llu)\n", argv[a], rc, rc2,
                    (unsigned long long)marks, (unsigned long long)pb.n_reads, (unsigned long long)pr.n_reads, (unsigned long long)flushed_bases, (unsigned long long)pr.n_bases);
            return 1;
        }
        printf("%d %llu %llu %llu %llu %llu\n", rc, (unsigned long long)pr.n_seg(), (unsigned long long)pr.n_bases, (unsigned long long)pr.n_reads,
               (unsigned long long)pr.n_input_bases, (unsigned long long)sum);
        free(exact);
    }
    printf("ok: %d texts\n", argc - 2);
    return 0;
}
