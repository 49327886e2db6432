// The BGZF block encoder of csrc/deflate_write.h alone, as a stand-alone program (tests/test_deflate_write_host.py builds it
// with AddressSanitizer and UBSan): the catalogue of tests/bgzf_write_cases.py, generated here, compressed by the shared
// encoder and inflated again with zlib inside the program; the code lengths, the checksum arithmetic and the framing.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include <zlib.h>

#include "deflate_write.h"

using namespace shk;

static int failures = 0;
#define CHECK(c, ...) do { if (!(c)) { failures++; printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #c); printf(__VA_ARGS__); printf("\n"); } } while (0)

static uint64_t rng_state = 88172645463325252ull;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 16); }

static std::vector<uint8_t> acgt_lines(size_t n, size_t width = 60) {
    std::vector<uint8_t> t(n);
    for (size_t i = 0; i < n; i++) t[i] = (i % (width + 1)) == width ? (uint8_t)'\n' : (uint8_t)"ACGT"[rnd() & 3u];
    return t;
}
static std::vector<uint8_t> from_counts(const std::vector<uint32_t> &counts) {
    std::vector<uint8_t> t;
    for (size_t i = 0; i < counts.size(); i++) t.insert(t.end(), counts[i], (uint8_t)(40 + i));
    for (size_t i = t.size(); i > 1; i--) std::swap(t[i - 1], t[rnd() % i]);
    return t;
}

// every member of a BGZF file, one after the other, with zlib; the framing on the way
static bool inflate_file(const std::vector<uint8_t> &f, std::vector<uint8_t> &text, size_t &members, std::string &why) {
    text.clear(); members = 0;
    size_t at = 0;
    while (at < f.size()) {
        if (f.size() - at < 28) { why = "a tail too short for a block"; return false; }
        const uint8_t *h = f.data() + at;
        if (h[0] != 0x1f || h[1] != 0x8b || h[2] != 8 || h[3] != 4 || h[10] != 6 || h[11] != 0 || h[12] != 'B' || h[13] != 'C' || h[14] != 2 || h[15] != 0) { why = "header"; return false; }
        const size_t bsize = (size_t)(h[16] | (h[17] << 8)) + 1;
        if (at + bsize > f.size()) { why = "BSIZE past the end"; return false; }
        z_stream z; memset(&z, 0, sizeof z);
        if (inflateInit2(&z, 15 + 16) != Z_OK) { why = "inflateInit2"; return false; }
        std::vector<uint8_t> out(DW_BLOCK_TEXT + 1);
        z.next_in = const_cast<uint8_t *>(h); z.avail_in = (uInt)bsize;
        z.next_out = out.data(); z.avail_out = (uInt)out.size();
        const int rc = inflate(&z, Z_FINISH);
        const size_t got = out.size() - z.avail_out, used = bsize - z.avail_in;
        inflateEnd(&z);
        if (rc != Z_STREAM_END) { why = "zlib refuses the member: " + std::to_string(rc); return false; }      // (gzip mode: CRC-32 and ISIZE are checked by zlib)
        if (used != bsize) { why = "the member does not end where BSIZE says"; return false; }
        if (got > DW_BLOCK_TEXT) { why = "a block of more than 65280 bytes"; return false; }
        text.insert(text.end(), out.begin(), out.begin() + (long)got);
        at += bsize; members++;
    }
    return true;
}

static void check_text(const char *name, const std::vector<uint8_t> &text, int want_btype) {
    std::vector<uint8_t> file(dw_host_file_bound(text.size()));
    const size_t n = dw_host_file(text.data(), text.size(), file.data());
    CHECK(n <= file.size(), "%s: %zu bytes written, room for %zu", name, n, file.size());
    file.resize(n);
    std::vector<uint8_t> back; size_t members = 0; std::string why;
    const bool ok = inflate_file(file, back, members, why);
    CHECK(ok, "%s: %s", name, why.c_str());
    CHECK(back == text, "%s: the inflated bytes differ", name);
    CHECK(members == dw_n_blocks(text.size()) + 1, "%s: %zu members", name, members);
    CHECK(n >= DW_EOF_BYTES, "%s", name);
    for (uint32_t i = 0; i < DW_EOF_BYTES && n >= DW_EOF_BYTES; i++) CHECK(file[n - DW_EOF_BYTES + i] == dw_bgzf_eof_byte(i), "%s: end marker byte %u", name, i);
    if (want_btype >= 0 && !text.empty()) CHECK(((file[18] >> 1) & 3) == want_btype, "%s: BTYPE %d", name, (file[18] >> 1) & 3);
    std::vector<uint8_t> again(dw_host_file_bound(text.size()));
    again.resize(dw_host_file(text.data(), text.size(), again.data()));
    CHECK(again == file, "%s: not deterministic", name);
}

static void check_lengths(const char *name, const uint32_t *counts) {
    DwScratch s; uint8_t len[DW_LIT];
    dw_rank(counts, DW_LIT, s.order, 0, 1);
    const int used = dw_lengths(counts, DW_LIT, 15, s, len);
    uint32_t kraft = 0; int n = 0;
    for (int i = 0; i < DW_LIT; i++) {
        CHECK(len[i] <= 15 && (len[i] != 0) == (counts[i] != 0), "%s: symbol %d length %d count %u", name, i, len[i], counts[i]);
        if (len[i]) { kraft += 1u << (15 - len[i]); n++; }
    }
    CHECK(n == used, "%s", name);
    if (used >= 2) CHECK(kraft == 1u << 15, "%s: Kraft sum %u / 32768", name, kraft);
    // the ranks of dw_rank by several lanes are the ranks by one
    DwScratch s2;
    for (int lane = 0; lane < 64; lane++) dw_rank(counts, DW_LIT, s2.order, lane, 64);
    CHECK(memcmp(s.order, s2.order, sizeof(uint16_t) * (size_t)used) == 0, "%s: the ranks depend on who sorts", name);
}

int main() {
    // ---- the checksum arithmetic against zlib
    {
        const std::vector<uint8_t> t = acgt_lines(70000);
        for (size_t cut : {(size_t)0, (size_t)1, (size_t)1024, (size_t)65279, (size_t)70000}) {
            const uint32_t a = (uint32_t)crc32(0, t.data(), (uInt)cut), b = (uint32_t)crc32(0, t.data() + cut, (uInt)(t.size() - cut));
            CHECK(dw_crc_join(a, b, t.size() - cut) == (uint32_t)crc32(0, t.data(), (uInt)t.size()), "cut %zu", cut);
        }
        CHECK(dw_crc_entry(1) == 0x77073096u && dw_gf_x8n(0) == 0x80000000u, "table entry / x^0");
    }
    // ---- the order of the code-length code lengths
    {
        static const int want[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
        for (int i = 0; i < 19; i++) CHECK(dw_cl_order(i) == want[i], "position %d", i);
    }
    // ---- the code lengths
    {
        uint32_t c[DW_LIT];
        for (int round = 0; round < 300; round++) {
            memset(c, 0, sizeof c);
            const int used = round % 10 == 0 ? 1 : 1 + (int)(rnd() % 256);
            for (int j = 0; j < used; j++) c[rnd() % 256] = round % 3 == 0 ? 5u : (round % 3 == 1 ? 1u + rnd() % 1000u : 1u << (rnd() % 16));
            c[DW_EOB] = 1;
            check_lengths("random histogram", c);
        }
        memset(c, 0, sizeof c);
        uint32_t p = 1;
        for (int i = 0; i < 20; i++) { c[100 + i] = p; p *= 3; }      // 21 deep whatever the ties
        c[DW_EOB] = 1;
        check_lengths("powers of three", c);
        memset(c, 0, sizeof c);
        c[7] = 9;
        check_lengths("a lone symbol", c);
    }
    // ---- the catalogue
    check_text("empty", {}, -1);
    check_text("one byte", {(uint8_t)'A'}, 0);
    check_text("acgt 65279", acgt_lines(65279), 2);
    check_text("acgt 65280", acgt_lines(65280), 2);
    check_text("acgt 65281", acgt_lines(65281), 2);
    check_text("one value", std::vector<uint8_t>(65280, (uint8_t)'G'), 2);
    { std::vector<uint32_t> flat(256, 255); std::vector<uint8_t> t = from_counts(flat); for (auto &b : t) b = (uint8_t)(b - 40); check_text("all values in equal numbers", t, 0); }
    { std::vector<uint8_t> t(65280 + 4000); for (auto &b : t) b = (uint8_t)rnd(); check_text("random bytes", t, 0); }
    { std::vector<uint32_t> f = {1, 1}; while (f.size() < 22) f.push_back(f[f.size() - 1] + f[f.size() - 2]); check_text("fibonacci", from_counts(f), 2); }
    { std::vector<uint32_t> f = {1, 1, 3, 4}; while (f.size() < 22) f.push_back(f[f.size() - 1] + f[f.size() - 2]); check_text("lucas", from_counts(f), 2); }
    {
        std::string gfa = "H\tVN:Z:1.0\n";
        for (int i = 1; i <= 40; i++) { gfa += "S\t" + std::to_string(i) + "\t"; for (int j = 0; j < 100 + i; j++) gfa += "ACGT"[rnd() & 3u]; gfa += "\tLN:i:" + std::to_string(100 + i) + "\tKC:i:" + std::to_string(700 + i) + "\n"; }
        for (int i = 1; i < 40; i++) gfa += "L\t" + std::to_string(i) + "\t+\t" + std::to_string(i + 1) + "\t-\t14M\n";
        check_text("GFA", std::vector<uint8_t>(gfa.begin(), gfa.end()), 2);
        std::string dot = "digraph sparrowhawk {\n";
        for (int i = 1; i <= 40; i++) dot += "  \"" + std::to_string(i) + "\" [label=\"" + std::to_string(i) + " len=" + std::to_string(100 + i) + " kc=7\"];\n";
        dot += "}\n";
        check_text("DOT", std::vector<uint8_t>(dot.begin(), dot.end()), 2);
        std::vector<uint8_t> three = acgt_lines(65280 + 777);
        for (int i = 0; i < 3; i++) three.insert(three.end(), gfa.begin(), gfa.end());
        const std::vector<uint8_t> more = acgt_lines(65280, 80);
        three.insert(three.end(), more.begin(), more.end());
        three.resize(2 * 65280 + 12345);
        check_text("three blocks", three, 2);
    }
    if (failures) { printf("%d checks failed\n", failures); return 1; }
    printf("ok: deflate_write.h\n");
    return 0;
}
