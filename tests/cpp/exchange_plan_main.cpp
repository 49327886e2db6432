// exchange_plan_main.cpp — csrc/exchange_plan.h without a GPU and without Python in the process: reads cases from the file
// named on the command line, one per line, and prints what the header's functions give, one line per result
// (tests/test_exchange_plan_host.py writes the cases and compares).  Built with AddressSanitizer and UBSan.
//   choose  total world per_part                          -> choose P
//   plan    world P rank  counts[world * P]               -> plan rc, then owned / base / send / recv / run_off / run_cnt
//   verdict world P rank  per rank: send[P] raw[P] failed mode
//                                                         -> rows (filled, read back), verdict peer_failed weighted, counts,
//                                                            raw_counts, fit
//   bytes   world P rank elem  counts[world * P]          -> send_off / send_bytes / recv_off / recv_bytes / n n_send n_recv
//   gather  world  rows[world]                            -> off8 / len8 / off4 / len4 / total
//   histo   counted failed in_reads                       -> histo <message, or nothing>
#include <stdio.h>
#include <stdlib.h>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "exchange_plan.h"

using namespace shk;

template <typename T> static void line(const char *name, const std::vector<T> &v) {
    std::cout << name;
    for (const T &x : v) std::cout << ' ' << (unsigned long long)x;
    std::cout << '\n';
}
static std::vector<uint64_t> take(std::istringstream &in, size_t n) {
    std::vector<uint64_t> v(n);
    for (uint64_t &x : v) if (!(in >> x)) { fprintf(stderr, "short case\n"); exit(2); }
    return v;
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: exchange_plan_main CASES\n"); return 2; }
    std::ifstream f(argv[1]);
    std::string text;
    while (std::getline(f, text)) {
        std::istringstream in(text);
        std::string what;
        if (!(in >> what)) continue;
        if (what == "choose") {
            const auto a = take(in, 3);
            std::cout << "choose " << choose_partitions(a[0], (uint32_t)a[1], a[2]) << '\n';
        } else if (what == "plan" || what == "bytes") {
            const auto a = take(in, what == "bytes" ? 4 : 3);
            const uint32_t world = (uint32_t)a[0], P = (uint32_t)a[1], rank = (uint32_t)a[2];
            const auto counts = take(in, (size_t)world * P);
            ExchangePlan pl; std::string err;
            const int rc = plan_exchange(counts.data(), world, P, rank, pl, err);
            if (what == "plan") {
                std::cout << "plan " << rc << '\n';
                if (rc) continue;
                line("owned", pl.owned); line("base", pl.base); line("send", pl.send_counts); line("recv", pl.recv_counts);
                line("run_off", pl.run_off); line("run_cnt", pl.run_cnt);
            } else {
                if (rc) { fprintf(stderr, "bytes: the plan failed\n"); return 2; }
                const ExchangeBytes x = exchange_bytes(pl, a[3]);
                line("send_off", x.send_off); line("send_bytes", x.send_bytes); line("recv_off", x.recv_off); line("recv_bytes", x.recv_bytes);
                std::cout << "n " << x.n_send << ' ' << x.n_recv << '\n';
            }
        } else if (what == "verdict") {
            const auto a = take(in, 3);
            const uint32_t world = (uint32_t)a[0], P = (uint32_t)a[1], rank = (uint32_t)a[2];
            std::vector<uint64_t> rows, back;
            for (uint32_t r = 0; r < world; r++) {
                const auto send = take(in, P), raw = take(in, P), fm = take(in, 2);
                const std::vector<uint64_t> row = size_row_fill(P, send.data(), raw.data(), fm[0] != 0, fm[1]);
                if (row.size() != size_row_words(P)) { fprintf(stderr, "row size\n"); return 2; }
                rows.insert(rows.end(), row.begin(), row.end());
            }
            for (uint32_t r = 0; r < world; r++) {            // what a reader of row r sees, in the order the case gave it
                const SizeRow row = size_row_read(rows, P, r);
                back.insert(back.end(), row.send, row.send + P); back.insert(back.end(), row.raw, row.raw + P);
                back.push_back(row.failed ? 1 : 0); back.push_back(row.mode);
            }
            line("rows", back);
            const DedupeVerdict v = dedupe_verdict(rows, world, P);
            std::cout << "verdict " << (v.peer_failed ? 1 : 0) << ' ' << (v.weighted ? 1 : 0) << '\n';
            line("counts", v.counts); line("raw_counts", v.raw_counts);
            std::cout << "fit " << (raw_records_fit(v, world, P, rank) ? 1 : 0) << '\n';
        } else if (what == "gather") {
            const auto a = take(in, 1);
            const GatherLayout g = gather_layout(take(in, (size_t)a[0]));
            line("off8", g.off8); line("len8", g.len8); line("off4", g.off4); line("len4", g.len4);
            std::cout << "total " << g.n_total << '\n';
        } else if (what == "histo") {
            const auto a = take(in, 3);
            uint64_t tail[HT_WORDS];
            tail[HT_COUNTED] = a[0]; tail[HT_FAILED] = a[1]; tail[HT_IN_READS] = a[2];
            const std::string m = instances_mismatch(tail);
            std::cout << "histo" << (m.empty() ? "" : " ") << m << '\n';
        } else { fprintf(stderr, "unknown case %s\n", what.c_str()); return 2; }
    }
    return 0;
}
