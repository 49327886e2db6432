// ctl_words.h — the 32 device control words of a pipeline (Pipeline::ctl_), one typed layout per ERA.  An era begins where
// the host zeroes the whole buffer; within an era a word keeps one meaning (a union where the mode decides it).  The host
// addresses the words through these members only; the kernels take plain pointers and never see the structs.  The table of
// writers, readers and lifetimes is in DESIGN.md ("The pipeline's control words"); the slots are pinned below.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace shk {

static constexpr int CTL_WORDS = 32;

// Counting era: zeroed at the global count, at the start of pass 1, at every attempt of pass 2 and in filter().
// (a 64-bit member that a kernel takes as a 32-bit pointer is used in its low half only)
struct CountWords {
    union { unsigned long long row_cursor;             // rows emitted so far (pass 2, k_compact, k_compact_rows)
            unsigned long long g_instances; };         // global-count mode: k-mer instances (k_count_segments)
    union { unsigned long long instances;              // k-mer instances counted (pass 2)
            unsigned long long g_overflow; };          // global-count mode: the table was too small
    uint32_t part_too_large, bucket_splits;            // `flags` of k_count_partitions / k_count_buckets: residue splitting gave up; bucket rounds split (statistic)
    uint32_t n_handed_over, tally;                     // `ovf_n`: partitions listed in ovf[]; tried | overflowed << 16 of the sampled ones
    unsigned long long bucket_list_len;                // k_ovf_check: buckets listed for k_count_buckets
    unsigned long long spare5[4];
    unsigned long long bloom_keys;                     // pass 2, Bloom mode: distinct k-mers that reached a table (k_count_buckets)
    unsigned long long spare10;
    unsigned long long probe_work;                     // work counter of the fused k_count_partitions
    unsigned long long dedupe_work;                    // work counter of k_dedupe_partitions, then of the residue re-run
    unsigned long long spare13;
    uint32_t groups_out, group_tally;                  // k_count_weighted's `work_and_tally`; the high half starts at k_dedupe_partitions' verdict
    unsigned long long spare15[7];
    unsigned long long er_cursor;                      // EmitRanges::tab_cursor: rows << 32 | table slots reserved by the counting groups
    unsigned long long er_broken;                      // EmitRanges::broken: a group left in more than one piece
    unsigned long long spare24[8];
};
// Pass 1's flags (`flags` of k_partition: [0], [1] and, 64 bits wide, [2]).  They lie outside the 32 words: pass 2 may be
// launched behind pass 1 before the host has looked at them, and zeroes the words for its own era.
struct P1Words {
    uint32_t spare, seg_too_long;                      // [1]: a read segment beyond 32768 bases
    unsigned long long max_fill;                       // [2]: the fullest slice of pass 1
};
// What Pipeline::ctl_ holds during the counting era, and the image of it that ONE transfer brings to the host's mailbox at the
// wait of pass 2: the words, the histogram of pass 2, pass 1's flags.  The fill in front of pass 1 zeroes all of it; an attempt
// of pass 2 that does not follow pass 1 directly zeroes `w` and `hist`.  (The graph era uses the first 32 words only.)
struct CountMail {
    CountWords w;
    unsigned long long hist[500];                      // k_count_weighted / k_count_partitions / k_count_buckets: distinct k-mers by count
    P1Words p1;
};
static constexpr int COUNT_MAIL_WORDS = (int)(sizeof(CountMail) / 8);
static_assert(sizeof(CountMail) == (CTL_WORDS + 500 + 2) * 8 && offsetof(CountMail, hist) == CTL_WORDS * 8 && offsetof(CountMail, p1) == (CTL_WORDS + 500) * 8,
              "CountMail: words, histogram, pass 1's flags, contiguous");
static inline unsigned tally_tried(uint32_t t) { return t & 0xFFFFu; }
static inline unsigned tally_over(uint32_t t) { return t >> 16; }
static inline unsigned long long er_rows(unsigned long long cursor) { return cursor >> 32; }

// Graph era: zeroed at build_graph(); lasts through the correction, the collapse, the sharded assembly and the device writer.
struct GraphWords {
    unsigned long long spare0;                         // (read back with the two below, never written)
    unsigned long long table_flag;                     // k_graph_local: 1 a mini table overflowed, 2 a row outside its group's range
    unsigned long long slots_used;                     // k_gp_scan: slots of all mini tables
    unsigned long long n_cand, n_tips;                 // correction scratch of a round: tip candidates, tips walked
    union { unsigned long long tips_removed;           // correction rounds >= 1
            unsigned long long n_splitters; };         // rank_chains: k_succ_split, appended to by k_orphan_cycles
    union { unsigned long long bubbles_removed;        // correction rounds >= 1
            unsigned long long n_chains; };            // rank_chains: chains reported (k_rank_tails)
    unsigned long long n_ring_splitters;               // splitters that sit on a circular unitig (statistic)
    uint32_t collapse_flag, n_spl_wanted;              // `flags` of the collapse: 2 / 3 / 4 ...; the splitter count that did not fit
    unsigned long long n_alive;                        // alive oriented nodes (k_succ_split)
    unsigned long long n_walked;                       // nodes covered by the fragment walk (k_walk_frags)
    unsigned long long n_fork_cand;                    // correction scratch of a round: fork candidates (k_fork_candidates; a word of its own, so that one fill opens a round)
    unsigned long long spare12;
    union { unsigned long long xq_count;               // build_graph, sharded: neighbour queries that go to other ranks
            unsigned long long halflink_flags; };      // shard_assemble: k_hl_apply / k_ls_answer found the ranks disagreeing
    unsigned long long writer_flag;                    // k_w_plan_fill: a contig beyond 2^32 bases
    unsigned long long spare15;
    unsigned long long r0_tips_removed, r0_bubbles_removed;   // correction round 0; the collapse's `skip` reads the pair
    unsigned long long plan_state, plan_bytes, plan_emitted;  // k_plan_emit's `plan`: 1 done / 2 not planned, bytes of text, chains emitted
    unsigned long long spare21[11];
};

#define SHK_CTL_AT(S, m, slot, half) static_assert(offsetof(S, m) == (slot) * 8 + (half) * 4, #S "::" #m " moved")
static_assert(sizeof(CountWords) == CTL_WORDS * 8 && sizeof(GraphWords) == CTL_WORDS * 8, "32 control words");
SHK_CTL_AT(CountWords, row_cursor, 0, 0);     SHK_CTL_AT(CountWords, g_instances, 0, 0);
SHK_CTL_AT(CountWords, instances, 1, 0);      SHK_CTL_AT(CountWords, g_overflow, 1, 0);
SHK_CTL_AT(CountWords, part_too_large, 2, 0); SHK_CTL_AT(CountWords, bucket_splits, 2, 1);
SHK_CTL_AT(CountWords, n_handed_over, 3, 0);  SHK_CTL_AT(CountWords, tally, 3, 1);
SHK_CTL_AT(CountWords, bucket_list_len, 4, 0);
SHK_CTL_AT(CountWords, bloom_keys, 9, 0);
SHK_CTL_AT(CountWords, probe_work, 11, 0);    SHK_CTL_AT(CountWords, dedupe_work, 12, 0);
SHK_CTL_AT(CountWords, groups_out, 14, 0);    SHK_CTL_AT(CountWords, group_tally, 14, 1);
SHK_CTL_AT(CountWords, er_cursor, 22, 0);     SHK_CTL_AT(CountWords, er_broken, 23, 0);
SHK_CTL_AT(GraphWords, spare0, 0, 0);         SHK_CTL_AT(GraphWords, table_flag, 1, 0);
SHK_CTL_AT(GraphWords, slots_used, 2, 0);     SHK_CTL_AT(GraphWords, n_cand, 3, 0);
SHK_CTL_AT(GraphWords, n_tips, 4, 0);
SHK_CTL_AT(GraphWords, tips_removed, 5, 0);   SHK_CTL_AT(GraphWords, n_splitters, 5, 0);
SHK_CTL_AT(GraphWords, bubbles_removed, 6, 0); SHK_CTL_AT(GraphWords, n_chains, 6, 0);
SHK_CTL_AT(GraphWords, n_ring_splitters, 7, 0);
SHK_CTL_AT(GraphWords, collapse_flag, 8, 0);  SHK_CTL_AT(GraphWords, n_spl_wanted, 8, 1);
SHK_CTL_AT(GraphWords, n_alive, 9, 0);        SHK_CTL_AT(GraphWords, n_walked, 10, 0);
SHK_CTL_AT(GraphWords, n_fork_cand, 11, 0);
SHK_CTL_AT(GraphWords, xq_count, 13, 0);      SHK_CTL_AT(GraphWords, halflink_flags, 13, 0);
SHK_CTL_AT(GraphWords, writer_flag, 14, 0);
SHK_CTL_AT(GraphWords, r0_tips_removed, 16, 0); SHK_CTL_AT(GraphWords, r0_bubbles_removed, 17, 0);
SHK_CTL_AT(GraphWords, plan_state, 18, 0);    SHK_CTL_AT(GraphWords, plan_bytes, 19, 0);
SHK_CTL_AT(GraphWords, plan_emitted, 20, 0);
#undef SHK_CTL_AT

}  // namespace shk
