// fasta_slices_main.cpp — the FASTA record-start rule (csrc/fastq.cpp: fasta_first_record_start, fasta_last_record_start,
// fasta_slice_bounds) as a stand-alone program, for a build with AddressSanitizer and UBSan (tests/test_fasta_slices.py).
// Every text lies in an exact-size heap block, so a read one byte in front of it or behind it is a finding.  The hand cases
// first, then every `from` and every prefix of a small text against a byte-by-byte restatement of the rule.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>

#include "fastq.h"

using namespace shk;

static const uint64_t NONE = UINT64_MAX;
static int failures = 0;

struct Exact {                                            // the text in a heap block of exactly its size
    uint8_t *p; size_t n;
    explicit Exact(const std::string &s) : p((uint8_t *)malloc(s.size() ? s.size() : 1)), n(s.size()) { if (!p) abort(); memcpy(p, s.data(), s.size()); }
    ~Exact() { free(p); }
};

static bool starts(const uint8_t *t, size_t p) { return t[p] == '>' && (p == 0 || t[p - 1] == '\n'); }
static uint64_t model_first(const uint8_t *t, size_t n, size_t from) { for (size_t p = from; p < n; p++) if (starts(t, p)) return p; return NONE; }
static uint64_t model_last(const uint8_t *t, size_t n) { for (size_t p = n; p-- > 0;) if (starts(t, p)) return p; return NONE; }

static void expect(const char *what, uint64_t got, uint64_t want) {
    if (got != want) { fprintf(stderr, "%s: got %llu, want %llu\n", what, (unsigned long long)got, (unsigned long long)want); failures++; }
}
static void first_is(const std::string &s, size_t from, uint64_t want) {
    Exact e(s);
    expect(("first(" + s + ")").c_str(), fasta_first_record_start(e.p, e.n, from), want);
}
static void last_is(const std::string &s, uint64_t want) {
    Exact e(s);
    expect(("last(" + s + ")").c_str(), fasta_last_record_start(e.p, e.n), want);
}
static void bounds_are(const std::string &s, uint32_t rank, uint32_t world, uint64_t c0, uint64_t c1, uint64_t w0, uint64_t w1) {
    Exact e(s);
    uint64_t s0 = 77, s1 = 77;
    fasta_slice_bounds(e.p, e.n, rank, world, c0, c1, s0, s1);
    expect("slice begin", s0, w0); expect("slice end", s1, w1);
}

int main() {
    // n = 0, from = n
    first_is("", 0, NONE); last_is("", NONE);
    first_is(">a\nAC\n", 6, NONE);
    bounds_are("", 0, 1, 0, 0, 0, 0); bounds_are("", 1, 3, 0, 0, 0, 0);
    // '>' as byte 0, '>' as the last byte
    first_is(">", 0, 0); last_is(">", 0);
    first_is(">a\nAC\n", 0, 0); last_is(">a\nAC\n", 0);
    first_is(">a\nAC\n>", 1, 6); last_is(">a\nAC\n>", 6);
    first_is("AC>", 0, NONE); last_is("AC>", NONE);          // (behind no newline)
    // from on, before and after a header
    const std::string t = ">a\nAC\n>b x>y\nA>C\n\r\n>c\r\nGT";
    const size_t b = t.find(">b"), c = t.find(">c");
    first_is(t, b, b); first_is(t, b - 1, b); first_is(t, b + 1, c); first_is(t, c, c); first_is(t, c + 1, NONE);
    last_is(t, c); last_is(t.substr(0, c), b); last_is(t.substr(0, c + 1), c); last_is(t.substr(0, b), 0);
    // a lone '\r' ends no line; "\r\n" does
    first_is("A\r>x\n", 0, NONE); first_is("A\r\n>x\n", 0, 3);
    // slices: s_0 = 0, s_world = e, in between the first start at or after the cut, e where there is none
    bounds_are(t, 0, 3, 0, b - 1, 0, b);
    bounds_are(t, 1, 3, b - 1, b + 1, b, c);
    bounds_are(t, 2, 3, b + 1, 999, c, t.size());
    bounds_are(t, 1, 3, c + 1, c + 2, t.size(), t.size());    // (an empty slice behind the last header)
    bounds_are("ACGT\nACGT\n", 1, 2, 5, 10, 10, 10);          // (no header at all: everything lies in slice 0)
    // every `from` of every prefix, against the restatement
    for (size_t n = 0; n <= t.size(); n++) {
        Exact e(t.substr(0, n));
        expect("last of a prefix", fasta_last_record_start(e.p, e.n), model_last(e.p, e.n));
        for (size_t from = 0; from <= n; from++) expect("first of a prefix", fasta_first_record_start(e.p, e.n, from), model_first(e.p, e.n, from));
    }
    if (failures) return 1;
    printf("ok\n");
    return 0;
}
