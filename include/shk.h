/*
 * shk.h — C ABI of libshk_hip.so: the MI355X (gfx950) implementation of the sparrowhawk-asm
 * assembly path (k-mer count -> filter -> de Bruijn graph -> correct -> collapse -> contigs).
 *
 * This is the drop-in boundary: exactly what a Rust `AssemblyHelper` (the wasm-bindgen struct
 * the reference's worker drives, /root/reference/www/src/workers/Assembler.ts:15-39) binds over
 * FFI.  See INTEGRATION.md for the Rust-side `extern "C"` block.  Plain pointers and sizes only;
 * no C++ or torch types cross this boundary.
 *
 * Threading: a handle is not thread-safe; one handle drives one HIP device (the current device
 * at shk_new time).  Every function returns SHK_OK (0) or a negative error code and never
 * aborts; the message is available from shk_last_error().  Strings returned by the library are
 * owned by the handle and stay valid until the next call on it or shk_free().
 *
 * There is no CPU fallback: without a usable HIP device shk_new() fails with SHK_E_DEVICE.
 */
#ifndef SHK_H
#define SHK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SHK_OK 0
#define SHK_E_PARAM  (-1)  /* even k, k out of range, bad argument                         */
#define SHK_E_STATE  (-2)  /* call out of order (Assembler.ts:92-111,121-139 call sequence) */
#define SHK_E_PARSE  (-3)  /* malformed FASTQ / gzip                                        */
#define SHK_E_OOM    (-4)  /* host or device memory                                         */
#define SHK_E_DEVICE (-5)  /* no HIP device / HIP runtime error                             */
#define SHK_E_INTERNAL (-6)

#define SHK_HISTO_BINS 500 /* KmerHistogram.vue:45 */
#define SHK_K_MIN 15
#define SHK_K_MAX 255      /* compiled key widths: 1..8 64-bit words (SPEC S3; docs/src/assembly.md:13 "up until 255", the UI offers 21..89) */

typedef struct shk_handle shk_handle;

/* Progress hook — replaces the crate's post_state(&str) -> postMessage({assemblyState})
 * (/root/reference/AGENTS.md:236-250; strings: AssemblyPage.vue:458-609).  Fires on the
 * calling thread. */
typedef void (*shk_progress_cb)(const char *state, void *user);

/* AssemblyHelper::new(k, verbose, min_count, min_qual, chunk_size, do_bloom, do_fit,
 *                     no_bubble_collapse, no_dead_end_removal)        Assembler.ts:15-29,94-99
 * Same nine parameters, same order.  Returns NULL on failure; shk_new_error() tells why.
 * verbose: results never depend on it.  A verbose handle also records per-stage HIP-event timers (shk_get_timings) and keeps
 * the initial adjacency bytes for shk_get_adjacency; a quiet one times the two counting passes only — an event between two
 * kernels costs the GPU ~10 us — and drops what only the inspection reads (SHK_STAGE_TIMERS=1 / SHK_KEEP_STAGES=1 turn
 * either on for quiet handles). */
shk_handle *shk_new(uint32_t k, int verbose, uint32_t min_count, uint32_t min_qual,
                    uint64_t chunk_size, int do_bloom, int do_fit,
                    int no_bubble_collapse, int no_dead_end_removal);
int shk_new_error(void);                 /* error code of the last failed shk_new on this thread */
const char *shk_new_error_message(void);

void shk_free(shk_handle *h);            /* Assembler.ts:141-143 (resetAll drops the handle) */
const char *shk_last_error(shk_handle *h);
void shk_set_progress_cb(shk_handle *h, shk_progress_cb cb, void *user);

/* AssemblyHelper::preprocess(file1, file2|null)                        Assembler.ts:35,100
 * fq1/fq2: whole FASTQ files in memory, plain or gzip (fastx_wasm.rs:9,53-70); fq2 may be NULL.
 * gzip: a file of >= 4 MiB (SHK_GUNZIP_DEVICE_MIN) that is one plain member, or a BGZF (bgzip) chain of blocks from its
 * first byte to its last, is inflated on the device (a BGZF file one wave per block), a plain member or a BGZF file in any
 * combination within a pair; everything else (several plain members, a broken chain, damaged data) is read on the host,
 * which owns the error messages.  SHK_GUNZIP_DEVICE=0: always on the host.
 * BGZF input of more text than one batch holds, or of 4 GiB and more a file, is inflated, parsed and counted on the device
 * window by window: runs of blocks of at most SHK_GUNZIP_DEVICE_WINDOW bytes of text (default 1 GiB, a value not yet chosen from a measured sweep: DESIGN.md §5; where it is set, a
 * file beyond it goes this way whatever its size), planned from the blocks' trailers before anything is uploaded.  A window
 * that is damaged or not regular 4-line FASTQ sends the rest of its file to the host reader.
 * The buffers are not retained. */
int shk_preprocess(shk_handle *h, const uint8_t *fq1, size_t n1, const uint8_t *fq2, size_t n2);

/* The same for FASTA input (SPEC S1a): whole files, plain text or gzip; fa2 may be NULL, two files are pooled, file 1 first.
 * A record is a header line ('>') and the lines behind it, joined; its segments are the maximal runs of ACGTacgt, a run of
 * more than 16384 + k - 1 bases goes in as overlapping pieces; min_qual is not used.  The results are those of shk_preprocess
 * on the FASTQ text in which every record stands with its joined sequence and a quality that passes.  State rules, progress
 * strings (loop:<records>:<pct>), bulk / chunked / Bloom modes (chunk_size counts records) as shk_preprocess.
 * Routes: a plain gzip member or a BGZF file the device inflater takes (>= SHK_GUNZIP_DEVICE_MIN) is inflated and packed on
 * the device; other gzip input is inflated on the host; text of >= SHK_FASTA_DEVICE_MIN bytes (default 1 MiB, the smallest size measured and already ahead there: DESIGN.md §5)
 * is uploaded and packed on the device by a byte-parallel packer (records of any length), smaller text and whatever the
 * device packer declines on the host, which owns the messages: a non-blank line in front of the first header of a file is
 * SHK_E_PARSE ("FASTA: ...").  SHK_HOST_PARSER=1: always the host packer.
 * Text beyond one batch (SHK_BATCH_BASES bytes) is cut on the host at header lines, a batch per piece; a single record beyond
 * one batch is SHK_E_PARAM.  shk_preprocess itself does not sniff FASTA and refuses it as before.
 * Timings: fasta_device_x1 / fasta_host_x1 (texts each packer took), fasta_batches_x1, fasta_device_parse_pack_host_clock. */
int shk_preprocess_fasta(shk_handle *h, const uint8_t *fa1, size_t n1, const uint8_t *fa2, size_t n2);

/* Streaming form of preprocess for inputs that do not fit host memory at once (modelled on the
 * reference's chunked bridge, rust/deacon-bridge/src/lib.rs:112,158).  Each chunk must hold
 * whole FASTQ records (plain text); shk_finish_reads() completes preprocessing. */
int shk_push_reads(shk_handle *h, const uint8_t *fastq_chunk, size_t n);
int shk_finish_reads(shk_handle *h);

/* Device-resident form of preprocess: reads already parsed, quality-masked, cut into valid
 * segments (SPEC S2) and 2-bit packed in HBM (layout: DESIGN.md "Data layout").
 *   d_bases   : uint32 words, base i of the stream in bits [2*(i%16), 2*(i%16)+1] of word i/16;
 *               at least ceil(n_bases/16)+1 words allocated
 *   d_seg_off : uint32[n_seg+1], base offset of each segment in the stream (ascending,
 *               d_seg_off[n_seg] == n_bases); every segment is >= k bases and of any length (a segment of more
 *               than 2048 k-mers is walked in pieces by the counting pass; before round 4 segments beyond 163840
 *               bases were refused)
 * Both are HIP device pointers on the handle's device; they are read, not retained.
 * n_reads is only used for progress/statistics. */
int shk_preprocess_packed_device(shk_handle *h, const void *d_bases, const void *d_seg_off,
                                 uint64_t n_seg, uint64_t n_bases, uint64_t n_reads);

/* The same reads, packed, in HOST memory (pinned memory makes the upload run at the link's rate): uploaded on the
 * handle's stream, then counted as shk_preprocess_packed_device does.  This is where SURVEY.md 8(d) starts the
 * clock of the throughput metric ("packed reads resident in host pinned memory"). */
int shk_preprocess_packed_host(shk_handle *h, const uint32_t *bases, const uint32_t *seg_off,
                               uint64_t n_seg, uint64_t n_bases, uint64_t n_reads);

/* AssemblyHelper::get_preprocessing_info() -> String                   Assembler.ts:36,110
 * JSON {"nkmers":int,"histo":[500 ints],"used_min_count":int}          Assembler.ts:1-5 */
const char *shk_get_preprocessing_info(shk_handle *h);

/* AssemblyHelper::assemble()                                           Assembler.ts:37,124 */
int shk_assemble(shk_handle *h);

/* AssemblyHelper::get_assembly() -> String                             Assembler.ts:38,127
 * JSON {"outfasta":str,"ncontigs":int,"outdot":str,"outgfa":str,"outgfav2":str}  :7-13 */
const char *shk_get_assembly(shk_handle *h);

/* ---- the outputs as BGZF (bgzip) files, compressed on the device (SPEC S11a; csrc/bgzf_write_gpu.hip).  No counterpart in
 * the reference's assembly path; its newer bridge has a compress_output switch for its results. */
#define SHK_OUT_FASTA 0
#define SHK_OUT_DOT   1
#define SHK_OUT_GFA1  2
#define SHK_OUT_GFA2  3
/* After shk_assemble: output `which` as a BGZF file whose inflated bytes are exactly the JSON field of shk_get_assembly()
 * ("outfasta", "outdot", "outgfa", "outgfav2") with its escapes undone.  Compressed on the device: one wave per block of
 * 65 280 bytes of text, literal-only dynamic-Huffman blocks (a stored block where that is not smaller), bgzip's end marker
 * behind the last; the bytes are deterministic.  *data is owned by the handle (valid until the next call on it or
 * shk_free).  SHK_E_STATE before shk_assemble, SHK_E_PARAM for another `which`.  An assembly with no contig gives the file
 * of the (possibly header-only) field.  Local, not collective: on a sharded assembly every rank may call it and gets the
 * same bytes.  Each file is made once per handle, at the first call that asks for it.
 * Timings: bgzf_out_files_x1 (files made), bgzf_out_from_device_x1 (of those, made from the device writer's JSON in HBM, no
 * upload), bgzf_out_text_MB, bgzf_out_file_MB, bgzf_out_kernels (where stage timers are on), bgzf_out_d2h_host_clock. */
int shk_get_assembly_bgzf(shk_handle *h, int which, const uint8_t **data, size_t *n);
/* Before shk_assemble (optional): the outputs that will be asked for, bit `which` each.  Where the JSON is written on the
 * device (csrc/writer_gpu.h / writer_text_gpu.h) the requested fields are then unescaped and compressed from HBM inside
 * shk_assemble, before that buffer is let go, and shk_get_assembly_bgzf returns them without any upload.  Mask 0 (the
 * default): shk_assemble does what it always did.  SHK_E_PARAM for a mask beyond 15, SHK_E_STATE after shk_assemble. */
int shk_request_assembly_bgzf(shk_handle *h, uint32_t mask);

/* ---- shard layer: one process per GPU (DESIGN.md "Multi-GPU").  It replaces the crate's rayon
 * read-parallel driver (north_star; not in the reference tree).  The
 * k-mer space is split by minimiser-hash partition: partition p belongs to rank p % world.
 * Sequence on every rank (collectives done by the caller, e.g. sparrowhawk_amd/dist.py):
 *   shk_shard_partition  reads -> super-k-mer records per partition; part_records[p] = records held
 *   shk_shard_pack       records copied densely to d_send at base_records[p] (caller's order)
 *        -- ONE all-to-all of d_send blocks (RCCL) --
 *   shk_shard_count      counts the owned partitions from d_recv; run tables [n_owned][n_sources]
 *                        give record offset/count of each source's run; local histogram out
 *        -- all-reduce of the 500-bin histogram and the instance count --
 *   shk_shard_rows       fit + filter on the global histogram; local solid rows (device pointers,
 *                        W key arrays + one count array, valid until shk_shard_set_solid)
 *        -- all-gather of the solid rows --
 *   shk_shard_set_solid  installs the whole solid set; the handle is then "preprocessed" and
 *                        shk_assemble() runs as usual (identically on every rank)
 * n_partitions: a power of two <= 16384, identical on all ranks. */
int shk_shard_partition(shk_handle *h, const void *d_bases, const void *d_seg_off, uint64_t n_seg,
                        uint64_t n_bases, uint64_t n_reads, uint32_t n_partitions,
                        uint64_t *part_records /* [n_partitions] out */);
uint32_t shk_shard_record_bytes(shk_handle *h);
int shk_shard_pack(shk_handle *h, void *d_send, const uint64_t *base_records, uint32_t n_partitions);
int shk_shard_count(shk_handle *h, const void *d_recv, const uint64_t *run_off, const uint32_t *run_cnt,
                    uint32_t n_owned, uint32_t n_sources, uint64_t *histo500_local,
                    uint64_t *n_instances_local);
int shk_shard_rows(shk_handle *h, const uint64_t *histo500_global, const void **d_keys /* [W] out */,
                   const void **d_cnt, uint64_t *n_rows, uint32_t *used_min_count);
int shk_shard_set_solid(shk_handle *h, const void *const *d_keys /* [W] */, const void *d_cnt,
                        uint64_t n_rows, uint64_t n_instances_global);

/* ---- the same sequence with the collectives INSIDE the library: RCCL over xGMI (librccl.so.1, opened on
 * first use).  One communicator per process and GPU.  The caller only distributes the 128-byte id that rank 0
 * obtains from shk_comm_unique_id() (ncclGetUniqueId) by whatever channel it has (MPI, a TCP store, a file),
 * then every rank — with its GPU current — calls shk_comm_init (ncclCommInitRank).  shk_shard_preprocess is
 * collective over the communicator: every rank calls it with its own share of the reads (n_seg may be 0) and
 * the same n_partitions (0 = chosen from the global instance count).  It runs
 *   pass 1 -> all-gather of the per-partition record counts (the size exchange) -> pack -> ONE pairwise
 *   exchange of the records (grouped ncclSend/ncclRecv) -> pass 2 over the owned partitions -> all-reduce
 *   of histogram + instance count (501 x u64) -> fit / filter -> all-gather of the solid rows -> install,
 * leaving every rank's handle "preprocessed".  By default the GRAPH STAYS SHARDED: every rank keeps the solid k-mers of
 * its own partitions, and shk_assemble() on these handles is COLLECTIVE over the same communicator (call it on every
 * rank; keep the communicator until it has returned): adjacency with one pairwise exchange of neighbour queries and one
 * of answers, non-branching paths contracted per rank and stitched across ranks, tips / bubbles on the graph of unitigs,
 * every rank writing the bases of its own k-mers into the contigs (csrc/shard_graph.h).  Every rank ends with the same
 * get_assembly() text; the stage-inspection getters then describe the rank's own rows.  From SHK_DEVICE_WRITER_MIN contigs
 * on (default 20 000, the knob of the one-GPU path) every rank writes that text on its GPU from the all-reduced contig
 * text, which is then never downloaded (csrc/writer_text_gpu.h, the writer behind shk_device_assembly_json;
 * SHK_SHARD_DEVICE_WRITER=0 keeps the host writer).  shk_get_timings then has "shard_writer_device_x1" = 1, the
 * "device_writer_*" entries and "outputs_host_clock" = 0; a rank whose device declines (no memory, a contig of 2^32 bases,
 * 2^31 contigs) reports "shard_writer_device_declined_x1" = 1 and runs the host writer alone — the same bytes.  With SHK_SHARD_GRAPH=0 in the
 * environment the solid set is gathered instead (all-gather of the solid rows) and shk_assemble() runs locally, on the
 * whole graph, on every rank.  A Rust host binds these five functions and never writes a collective itself. */
#define SHK_UNIQUE_ID_BYTES 128
typedef struct shk_comm shk_comm;
struct shk_packed;                       /* below: the host-side packer */
int shk_comm_unique_id(uint8_t id[SHK_UNIQUE_ID_BYTES]);
shk_comm *shk_comm_init(const uint8_t id[SHK_UNIQUE_ID_BYTES], int rank, int world);   /* NULL on failure */
const char *shk_comm_error(void);        /* message of the last failed shk_comm_* call on this thread */
int shk_comm_rank(const shk_comm *c);
int shk_comm_world(const shk_comm *c);
void shk_comm_free(shk_comm *c);
int shk_shard_preprocess(shk_handle *h, shk_comm *c, const void *d_bases, const void *d_seg_off, uint64_t n_seg,
                         uint64_t n_bases, uint64_t n_reads, uint32_t n_partitions);
/* The same call for a rank whose packed reads lie in HBM in SEVERAL batches (callers who stage reads themselves and hold 2^32
 * bases or more; the layer on which the file route below sits): batch b is d_bases[b] / d_seg_off[b] with n_seg[b] segments
 * and n_bases[b] < 2^32 bases, in the layout of shk_preprocess_packed_device; n_reads counts the reads of all of them.  Pass 1
 * runs on every batch into the same partitions, then everything goes on as in shk_shard_preprocess, which is this call with
 * one batch.  n_batches == 0: this rank has none.  The ranks need not hold the same number of batches.  Results do not depend
 * on how the reads were cut into batches.  The batches are not retained. */
int shk_shard_preprocess_batches(shk_handle *h, shk_comm *c, uint32_t n_batches, const void *const *d_bases, const void *const *d_seg_off,
                                 const uint64_t *n_seg, const uint64_t *n_bases, uint64_t n_reads, uint32_t n_partitions);
/* The same call from FASTQ FILES: every rank reads its share into ONE packed batch in HBM — inflated (csrc/inflate_gpu.hip)
 * and parsed (csrc/fastq_gpu.hip) on the device, so the compressed bytes are what crosses PCIe — and the batch goes through
 * shk_shard_preprocess as it is: the same progress strings, the same SHK_E_STATE rules, the handle ends "preprocessed", the
 * graph stays sharded by default and shk_assemble is collective as above.  Collective over c.
 *   split = 0: the buffers are this rank's OWN reads — plain text, a gzip member, BGZF, or a pair; fq1 == NULL && n1 == 0: this
 *              rank has none.
 *   split = 1: every rank passes the SAME file(s) and rank r takes slice r of `world` of each; the two files of a pair are
 *              sliced independently and pooled (SPEC S1).
 * The slice rule: with c_r the nominal cut — floor(r * n / world) in plain text and in the text of a plain gzip member, the
 * text offset at which a block begins in a BGZF chain (shk_plan_fastq_slices) — slice r is [s_r, s_(r+1)), s_0 = 0, s_world =
 * the end of the text without its trailing blank lines, and otherwise s_r = the first record start at or after c_r
 * (shk_host_first_record_start; the end where there is none).  Slices may be empty.
 * What crosses PCIe: of a BGZF file, the blocks of the rank's run, the one in front and a few behind (1 / world of the file:
 * the route that scales); of plain text, the slice.  A plain gzip member is inflated WHOLE by every rank, which then keeps its
 * slice: redundant work by construction — a deflate stream cannot be entered in the middle; compress with bgzip where the
 * ranks are many.  What the device declines (several members, a damaged block, text that is not regular 4-line FASTQ) is
 * read on the host, whole, and cut by the same rule; the host reader and the host parser own those messages, and the RECORD
 * NUMBERS in them count from the start of the rank's SLICE, not of the file.
 * A share of ANY size: one that fits one batch (SHK_BATCH_BASES, default 2^31 packed bases, at most 3 * 2^30) is read whole,
 * as described; a larger one goes through pass 1 batch by batch — a window is inflated and parsed, counted into the rank's
 * partitions, and let go — and everything behind pass 1 is the same (ONE record exchange).  Results do not depend on how a share
 * was cut.  Whether a share goes in batches is decided before anything is uploaded where the host can tell (the ISIZE sums of
 * the rank's run of BGZF blocks, the slice bounds of plain text).  In batches: a BGZF run is cut into windows of at most
 * SHK_GUNZIP_DEVICE_WINDOW (default 1 GiB, at most 2 * SHK_BATCH_BASES) bytes of text (shk_plan_share_windows), every window
 * but the last is cut at its last record start and the rest is carried, window w + 1 travels while window w is worked on;
 * plain text is cut on the host, at record starts, into pieces of about 2 * SHK_BATCH_BASES bytes; a plain gzip member is
 * inflated whole (on the host above 4 GiB of text) and the rank's slice of it is cut into such pieces on the device; the files
 * of a pair go one after the other.  A window that is not regular 4-line FASTQ goes to the host parser, from that window to the
 * end of the slice; its record numbers still count from the start of the slice.  One progress string
 * preprocess:<mode>:loop:<reads so far>:<pct> per batch (pct: the part of the share's text that is consumed; the last says 100).
 * The ranks need not agree: one may take several batches, another one, another none.
 * A rank whose reading fails (a parse error, a damaged stream, memory) still enters the next collective — the first one for a
 * share of one batch, the size exchange behind pass 1 for a failure in a later window: it returns its own code and message,
 * every other rank SHK_E_DEVICE "another rank failed during ...", and nobody hangs.  The environment switches that choose a
 * route (SHK_GUNZIP_DEVICE_MIN, ...) must be the same on every rank.  The buffers are not retained.
 * Timings: shard_fastq_batches_x1 (batches pass 1 took on this rank), shard_fastq_windows_x1 (windows and pieces of text they
 * were parsed from). */
int shk_shard_preprocess_fastq(shk_handle *h, shk_comm *c, const uint8_t *fq1, size_t n1, const uint8_t *fq2, size_t n2,
                               uint32_t n_partitions, int split);
/* The routes of split = 1 without a communicator (tests, staging; needs a GPU): slice `rank` of `world` of the file(s) as one
 * packed batch, copied back to the host (shk_packed_free).  *uploaded_bytes (optional): the compressed or text bytes that
 * crossed PCIe; *route (optional): "bgzf_slice", "member_whole", "text_slice" or "host" ('+' between two files that went
 * different ways) — on failure, the message. */
int shk_device_pack_fastq_slice(const uint8_t *fq1, size_t n1, const uint8_t *fq2, size_t n2, uint32_t k, uint32_t min_qual,
                                uint32_t rank, uint32_t world, struct shk_packed *out, uint64_t *uploaded_bytes, const char **route);
/* host-only: where those slices are cut — the smallest p >= from that begins a line, holds '@', and whose line after next
 * begins with '+' (the rule of shk_host_last_record_start, read forwards).  A line whose line after next has not begun inside
 * the text is undecided: the search stops there and never passes it over.  UINT64_MAX: none / undecided.
 * shk_device_first_record_start (needs a GPU): the device kernel that finds the same. */
uint64_t shk_host_first_record_start(const uint8_t *text, size_t n, uint64_t from);
int shk_device_first_record_start(const uint8_t *text, size_t n, uint64_t from, uint64_t *at);
/* The same call from FASTA FILES (SPEC S1a; shk_preprocess_fasta across ranks): the contract of shk_shard_preprocess_fastq —
 * collective over c, split = 0 (the rank's own files, or none) and split = 1 (slice r of the same files), the routes
 * (bgzf_slice, member_whole, text_slice, host), the SHK_E_STATE rules, one progress string
 * preprocess:<mode>:loop:<records so far>:<pct> per batch (the last says 100), the failure agreement (the failing rank returns
 * its own code and message, every other rank SHK_E_DEVICE "another rank failed during ...", nobody hangs); afterwards the handle
 * is "preprocessed", the graph stays sharded by default and shk_assemble is collective.  min_qual is not used; n_reads counts
 * records.
 * The slice rule: a record starts at p when text[p] == '>' and p begins a line (p == 0 or text[p - 1] == '\n'; a lone '\r'
 * ends no line).  s_0 = 0, s_world = the end of the text, otherwise s_r = the first record start at or after the nominal cut
 * c_r (the end where there is none), c_r as for FASTQ: floor(r * n / world) in plain text and in the text of a plain gzip
 * member, the block starts of shk_plan_fastq_slices in a BGZF chain.  Slices may be empty and records are never split; a
 * non-blank line in front of a file's first header lies in slice 0 and is SHK_E_PARSE ("FASTA: ...", the host packer's
 * message) there.  On the device the starts are found by a grid-wide search (csrc/inflate_gpu.hip: k_fasta_header_search).
 * What differs from FASTQ: a byte of text is a base, so a share goes in batches when its TEXT exceeds SHK_BATCH_BASES, and
 * every piece of text that becomes a batch is at most SHK_BATCH_BASES bytes, cut at the last header behind its first byte; a
 * single record beyond one batch is SHK_E_PARAM ("a single FASTA record of ... bytes exceeds one batch ...") on the rank that
 * meets it.  In a BGZF run a record beyond 16 MiB of carry, or a slice end not found within 16 MiB of follow-on blocks, sends
 * that file's slice from that window on to the host reader.  The two files of a pair are packed separately (the rule on the
 * lines in front of the first header holds for each file) and go to pass 1 as batches of their own.  Text that is inflated on
 * the device is packed there; host-resident text goes to the device packer from SHK_FASTA_DEVICE_MIN bytes of slice on and
 * to the host packer below it; SHK_HOST_PARSER=1 always takes the host packer, which also takes what the device packer
 * declines and owns the messages (record numbers count from the start of the slice).
 * Timings: shard_fasta_bgzf_slice_x1, shard_fasta_member_whole_x1, shard_fasta_text_slice_x1, shard_fasta_host_x1 (files by
 * route), shard_fasta_uploaded_bytes, shard_fasta_batches_x1, shard_fasta_windows_x1, shard_fasta_read_host_clock. */
int shk_shard_preprocess_fasta(shk_handle *h, shk_comm *c, const uint8_t *fa1, size_t n1, const uint8_t *fa2, size_t n2,
                               uint32_t n_partitions, int split);
/* The routes of split = 1 without a communicator (tests; needs a GPU), as shk_device_pack_fastq_slice: slice `rank` of
 * `world` of the file(s) as ONE packed batch on the host, the two files' batches concatenated.  A share beyond one batch is
 * SHK_E_PARAM. */
int shk_device_pack_fasta_slice(const uint8_t *fa1, size_t n1, const uint8_t *fa2, size_t n2, uint32_t k, uint32_t rank,
                                uint32_t world, struct shk_packed *out, uint64_t *uploaded_bytes, const char **route);
/* host-only: the FASTA record starts — first: the smallest p >= from with text[p] == '>' that begins a line; last: the
 * largest such p < n; UINT64_MAX: none.  shk_device_*_fasta_record_start (need a GPU): the device kernel that finds the same. */
uint64_t shk_host_first_fasta_record_start(const uint8_t *text, size_t n, uint64_t from);
uint64_t shk_host_last_fasta_record_start(const uint8_t *text, size_t n);
int shk_device_first_fasta_record_start(const uint8_t *text, size_t n, uint64_t from, uint64_t *at);
int shk_device_last_fasta_record_start(const uint8_t *text, size_t n, uint64_t *at);
/* host-only: the runs of blocks the ranks take of a BGZF chain.  isize[n_blocks] as for shk_plan_bgzf_windows; run r is the
 * blocks first_block[r] ... first_block[r + 1] - 1 and starts at the first block whose text offset is >= r * text / world;
 * first_block[0] = 0, first_block[world] = n_blocks; more ranks than blocks gives empty runs.  Returns world, or SHK_E_PARAM. */
int64_t shk_plan_fastq_slices(const uint32_t *isize, uint64_t n_blocks, uint32_t world, uint64_t *first_block /* [world + 1] */);
/* host-only: the exchange plan shk_shard_preprocess derives from the gathered record counts (exposed for the
 * CPU tests).  part_records_all: [world][n_partitions].  Outputs (caller-allocated): base [n_partitions],
 * send_counts / recv_counts [world], run_off / run_cnt [n_owned][world], n_owned = partitions p with
 * p % world == rank. */
int shk_plan_exchange(const uint64_t *part_records_all, uint32_t world, uint32_t n_partitions, uint32_t rank,
                      uint64_t *base, uint64_t *send_counts, uint64_t *recv_counts, uint64_t *run_off,
                      uint32_t *run_cnt);
uint32_t shk_choose_partitions(uint64_t total_instances_ub, uint32_t world, uint32_t key_words);
/* host-only: the windows shk_preprocess cuts a BGZF chain into that is too large to be inflated at once (exposed for
 * the CPU tests).  isize[n_blocks]: the blocks' ISIZE fields (0 ... 65536, empty blocks anywhere); budget: bytes of text
 * per window.  Window w is the blocks first_block[w] ... first_block[w + 1] - 1, the last one ends at n_blocks; every
 * window holds at most `budget` bytes of text and, unless the file has none, some.  Returns the number of windows (of
 * which the first `cap` are written), or SHK_E_PARAM when a block alone exceeds the budget. */
int64_t shk_plan_bgzf_windows(const uint32_t *isize, uint64_t n_blocks, uint64_t budget, uint64_t *first_block, uint64_t cap);
/* host-only: the windows ONE rank's run of blocks is cut into where its share exceeds one batch (shk_shard_preprocess_fastq):
 * shk_plan_fastq_slices, then shk_plan_bgzf_windows on the blocks of run `rank` alone.  first_block[w] counts blocks of the
 * FILE; the last window ends where the run ends (first_block[rank + 1] of shk_plan_fastq_slices); an empty run has no window.
 * Returns the number of windows (of which the first `cap` are written), or SHK_E_PARAM: rank >= world, an ISIZE beyond 65536,
 * a block of the run that alone exceeds the budget. */
int64_t shk_plan_share_windows(const uint32_t *isize, uint64_t n_blocks, uint32_t world, uint32_t rank, uint64_t budget,
                               uint64_t *first_block, uint64_t cap);
/* host-only: where such a window is cut — the start of the last FASTQ record of text[0..n) that is known to be one: a
 * line that begins with '@' and whose line after next begins with '+' (a quality line may begin with '@' too); a line
 * whose line after next has not begun inside the text is undecided and passed over.  UINT64_MAX: none.
 * shk_device_last_record_start (needs a GPU): the device kernel that finds the same on the uploaded window. */
uint64_t shk_host_last_record_start(const uint8_t *text, size_t n);
int shk_device_last_record_start(const uint8_t *text, size_t n, uint64_t *at);

/* ---- host-side packer (the parser the preprocess entry points use), exposed so a caller can
 * stage packed reads in HBM itself (bench.py, the multi-GPU shard layer). */
typedef struct shk_packed {
    uint32_t *bases;       /* ceil(n_bases/16)+1 words */
    uint32_t *seg_off;     /* n_seg+1 */
    uint64_t n_seg, n_bases, n_reads, n_input_bases;
} shk_packed;
/* returns SHK_OK or SHK_E_PARSE / SHK_E_OOM; *err (optional) receives a static message */
int shk_pack_fastq(const uint8_t *fq, size_t n, uint32_t k, uint32_t min_qual, shk_packed *out,
                   const char **err);
/* the host FASTA packer (SPEC S1a; plain or gzip): SHK_OK, SHK_E_PARSE (message with "FASTA") / SHK_E_OOM; SHK_E_PARAM
 * where k is not odd and within [15, 255] */
int shk_pack_fasta(const uint8_t *fa, size_t n, uint32_t k, shk_packed *out, const char **err);
/* the device FASTA packer alone (tests; needs a GPU), whatever the size of the text: the batch is copied back to the host.
 * *route (optional): "device", "host" (the device packer declined, the host packer took the text) — on failure, the message
 * ("host: <message>" where the host packer, having taken the text over, refused it). */
int shk_device_pack_fasta(const uint8_t *fa1, size_t n1, const uint8_t *fa2, size_t n2, uint32_t k, struct shk_packed *out,
                          const char **route);
void shk_packed_free(shk_packed *p);

/* ---- stage inspection (used by the parity tests; SURVEY.md §7 step 1 stages a-f).
 * All copy device state to caller-provided host arrays.  Key layout: W = ceil(2k/64) uint64
 * words per k-mer, w[0] least significant (SPEC S3).  Order of rows is unspecified. */
uint32_t shk_key_words(shk_handle *h);
uint64_t shk_total_instances(shk_handle *h);            /* valid k-mer windows counted (S4)   */
uint64_t shk_n_distinct(shk_handle *h);
int shk_get_distinct(shk_handle *h, uint64_t *keys, uint32_t *counts, uint64_t cap);
uint64_t shk_n_solid(shk_handle *h);
int shk_get_solid(shk_handle *h, uint64_t *keys, uint32_t *counts, uint64_t cap);
int shk_get_histo(shk_handle *h, uint64_t *histo500);
uint32_t shk_used_min_count(shk_handle *h);
/* after shk_assemble: per solid node (same row order as shk_get_solid) */
int shk_get_adjacency(shk_handle *h, uint8_t *adj_initial, uint8_t *adj_final, uint8_t *alive,
                      uint64_t cap);
/* timing of the last preprocess/assemble, milliseconds, by stage name; returns a JSON object.  Two entries are not times:
 * "peak_device_bytes" = the most device memory the handle held at once, "device_bytes_now" = what it holds at the call
 * (the reference reports the peak wasm memory with every assembly: Assembler.ts:69-71,137). */
const char *shk_get_timings(shk_handle *h);
/* the same figure alone: high-water mark of the device bytes charged to this handle (its pool blocks, the packed reads
 * uploaded for it, the exchange buffers of the shard layer) */
uint64_t shk_peak_device_bytes(shk_handle *h);
/* host-only (tests): the counter behind it — applies signed byte deltas in order, reports high-water mark and remainder */
void shk_host_mem_counter(const int64_t *deltas, size_t n, uint64_t *peak, uint64_t *current);

/* ---- host-only self tests of the device/host shared k-mer arithmetic (no GPU needed) */
int shk_host_canonical(const char *seq, uint32_t k, uint64_t *out_words /*W*/, int *orient);
uint64_t shk_host_nthash(const char *seq, uint32_t k);   /* canonical ntHash of seq[0..k) */
int shk_host_fit(const uint64_t *histo500, uint32_t *used_min_count); /* 1 ok, 0 fit failed */
/* the output writer alone (SPEC S10-S11: canonical strand, order, links, FASTA / DOT / GFA1 / GFA2, JSON) on
 * unitigs handed in as text, any strand, any order: seqs = the spellings back to back, offsets[n+1] their
 * bounds, kc[n] their k-mer count sums.  Returns a malloc'd NUL-terminated JSON (shk_host_free) or NULL. */
char *shk_host_assembly_json(const char *seqs, const uint64_t *offsets, const uint64_t *kc, uint64_t n_contigs, uint32_t k);
/* The device twin of shk_host_assembly_json (csrc/writer_text_gpu.h; needs a GPU): the same parameters, the same JSON byte
 * for byte.  It uploads the text and the arrays, runs the device writer from contig text alone on the current HIP device —
 * strand choice and reverse complement in place, order, links from a table of the contigs' end k-mers, records and
 * sequences — and returns a malloc'd NUL-terminated JSON (shk_host_free).  This is the writer the sharded shk_assemble
 * runs on the all-reduced contig text.  n_contigs == 0 gives the host twin's empty-assembly JSON.
 * NULL: bad parameters (the host twin's refusals: offsets not ascending, a contig shorter than k), out of device memory,
 * a contig of >= 2^32 bases, >= 2^31 contigs; *why (optional) says which. */
char *shk_device_assembly_json(const char *seqs, const uint64_t *offsets, const uint64_t *kc, uint64_t n_contigs, uint32_t k,
                               const char **why);
/* host-only (tests): the end keys of that writer, in the code the kernels share with the host (csrc/end_keys.h).
 * out_words[W] (W = ceil(2k/64), w[0] least significant) = seq[0..k) packed, reverse-complemented first if rc != 0;
 * *entry = the table word for that key with the given orientation and sorted position.  Of two entries with one key the
 * smaller word wins.  Returns SHK_OK or SHK_E_PARAM. */
int shk_host_end_key(const char *seq, uint32_t k, int rc, uint32_t orientation, uint32_t pos, uint64_t *out_words, uint64_t *entry);
/* the same on text that arrives while the writer works, piece_bytes at a time every delay_us microseconds (the device path
 * downloads the contigs in pieces and the writer copies what is there: csrc/pipeline.h TextArrival) — same JSON */
char *shk_host_assembly_json_arriving(const char *seqs, const uint64_t *offsets, const uint64_t *kc, uint64_t n_contigs, uint32_t k,
                                      uint64_t piece_bytes, uint32_t delay_us);
void shk_host_free(void *p);
/* host-only: the gzip reader of shk_preprocess alone (fastx_wasm.rs:53-70: gz sniff, multi-member) — BGZF blocks in
 * parallel, a large plain member by the multi-threaded two-pass inflater (csrc/inflate_mt.cpp), the rest by zlib.  *out is
 * malloc'd (shk_host_free); plain input is copied through.  *mt_members (optional): members the multi-threaded inflater
 * has handled in this process so far; *reader_seconds (optional): the time the reader itself took (without the copy into
 * *out).  SHK_GUNZIP_THREADS (environment): its thread count, 0 or 1 = zlib only. */
int shk_host_gunzip(const uint8_t *gz, size_t n, uint8_t **out, size_t *out_n, uint64_t *mt_members, double *reader_seconds);
/* the DEVICE inflater alone (csrc/inflate_gpu.hip; needs a GPU): shk_preprocess hands a plain gzip member or a BGZF
 * (bgzip) file of >= 4 MiB (SHK_GUNZIP_DEVICE_MIN) to it first — the compressed bytes are what crosses PCIe; a BGZF file is
 * decoded one wave per block — and reads on the host whatever it does not take.  0: *out (malloc'd, shk_host_free) holds
 * the bytes of the member or of the whole BGZF file, equal to zlib's; 1: not taken, *why (optional) says why; < 0: error.
 * *ms_total (optional): upload + kernels + checks.
 * Where SHK_GUNZIP_DEVICE_WINDOW is set, or the text of a BGZF file reaches 4 GiB, the file goes through the windows of
 * shk_preprocess (cut at record starts, the rest carried into the next window) and all its bytes come back. */
int shk_device_gunzip(const uint8_t *gz, size_t n, uint8_t **out, size_t *out_n, const char **why, double *ms_total);
/* ---- the BGZF block encoder alone (SPEC S11a; csrc/deflate_write.h: one header compiled for the kernels and for the host) */
/* host-only: code lengths for 257 counts (out[257], each 0..15, complete); SHK_E_PARAM when no count is > 0 or their sum
 * reaches 2^32.  A lone used symbol gets length 1. */
int shk_host_deflate_lengths(const uint32_t counts[257], uint8_t out[257]);
/* host-only: text as a BGZF file by the shared encoder (malloc'd, shk_host_free) */
int shk_host_bgzf_compress(const uint8_t *text, size_t n, uint8_t **out, size_t *out_n);
/* the same on the current HIP device (needs a GPU): byte for byte the host twin's file.  *ms_kernels optional. */
int shk_device_bgzf_compress(const uint8_t *text, size_t n, uint8_t **out, size_t *out_n, double *ms_kernels);
/* tests: the same on JSON string content, whose escapes (\n \t \" \\) the device undoes first (k_json_unesc_*: chunks of 2048
 * bytes, 8 consecutive bytes a thread); SHK_E_INTERNAL for any other byte behind a backslash, or a backslash at the end. */
int shk_device_bgzf_compress_escaped(const uint8_t *escaped, size_t n, uint8_t **out, size_t *out_n);
/* SPEC S9 (tips, bubbles) and S10 (chains of simple links, the circular cut) on UNITIG records instead of k-mers — what the
 * sharded assembly runs on every rank's host once the k-mer-level contraction is done on the GPUs (csrc/unitig_graph.h:
 * one record per strand of a unitig; first / last: [n_recs][W] words of its first / last k-mer as spelled; min_*: the
 * smallest oriented node of a record and its position, read for the records of rings only).  Exposed for the CPU tests.
 * Returns a malloc'd text (shk_host_free): "removed <tip nodes> <bubble nodes>", then one line per contig
 * "<ring> <rot> <nodes> <kc> : <record> <record> ...", "error: <what>" on inconsistent records, or NULL on bad parameters. */
char *shk_host_unitig_assemble(uint32_t k, uint64_t n_recs, const uint64_t *first, const uint64_t *last, const uint64_t *len,
                               const uint64_t *kc, const uint8_t *circ, const uint64_t *min_key, const uint8_t *min_o,
                               const uint64_t *min_pos, int tips, int bubbles);
/* The same on the current HIP device (csrc/unitig_graph_gpu.h: the index of chain starts, the links, the tip and bubble
 * rounds, the simple successors and the walk of the chains as kernels; only ring records go through the host's ring
 * loops.  SHK_UNITIG_CHAINS_DEVICE=0 (environment): the chains are walked by the host code from what comes back).  Same
 * parameters, the same text byte for byte, "error: ..." included; needs a GPU. */
char *shk_device_unitig_assemble(uint32_t k, uint64_t n_recs, const uint64_t *first, const uint64_t *last, const uint64_t *len,
                                 const uint64_t *kc, const uint8_t *circ, const uint64_t *min_key, const uint8_t *min_o,
                                 const uint64_t *min_pos, int tips, int bubbles);
/* The S10 walk alone, from arrays that are already settled: alive[r], mirror[r] (the record of r's mirror strand) and
 * succ[r] (the simple successor of an alive linear record, 0xFFFFFFFF: none); first: [n_recs][W] words.  The host walk
 * (unitig_chains) and its device twin (unitig_chains_device; needs a GPU) give the same malloc'd text (shk_host_free),
 * one line per contig in result order —
 *     linear:                  "0 <nodes> <kc> <text offset> : <record>@<node offset> ..."
 *     ring, before resolution: "1 <nodes> <kc> - : <record> ..."
 * — and a last line "need_min : <record> ...".  Text offsets are the running sum of nodes + k - 1 over the linear contigs
 * in front, node offsets the nodes of the contig's records in front.  Both check the arrays on the host first, with the
 * same code: "error: unitig chains: <what>" unless succ is none or an alive linear record, no two records share a
 * successor, mirror pairs up among the alive linear records, mirror[succ[r]] has mirror[r] as its successor, and dead and
 * circ records carry no successor.  The device entry reports "error: out of device memory" instead of falling back.
 * NULL on bad parameters. */
char *shk_host_unitig_chains(uint32_t k, uint64_t n_recs, const uint64_t *first, const uint64_t *len, const uint64_t *kc, const uint8_t *circ,
                             const uint8_t *alive, const uint32_t *mirror, const uint32_t *succ);
char *shk_device_unitig_chains(uint32_t k, uint64_t n_recs, const uint64_t *first, const uint64_t *len, const uint64_t *kc, const uint8_t *circ,
                               const uint8_t *alive, const uint32_t *mirror, const uint32_t *succ);

/* Device buffers of freed handles are cached process-wide for the next handle (a handle lives
 * for one preprocess+assemble); this returns the cache to the driver.  SHK_NO_POOL=1 disables it. */
void shk_release_cached_memory(void);

/* ---- test support: the block cache's fill-on-hand-out mode.  A block of the cache is never cleared: a buffer starts with what
 * its previous user left, and — a request is rounded up to 4 KiB (to 256 MiB above 256 MiB) and a cached block of up to
 * bytes + bytes/2 + 1 MiB may be handed out instead — ends in a tail nobody wrote.  With the mode on, every block is filled
 * with `word`, the whole rounded block, fresh or reused, before it is handed out, and so are the two device allocations that
 * do not come from the cache (the uploads of the host-buffer entry points, a communicator's stage buffer): the contents a
 * buffer starts with become an input a test chooses, and no result may depend on it.  Off by default, where it costs one
 * atomic load per hand-out.  The fill runs on the null stream and waits for the whole device, so the mode serialises the
 * handles of a process: it shows a dependence on stale memory, not a race.  SHK_POOL_FILL=<hex word> in the environment,
 * read once where SHK_NO_POOL is read, turns it on from the start (rank workers, tools).
 *   shk_debug_pool_fill          sets the mode for the process; returns the previous `on`
 *   shk_debug_pool_filled_bytes  the bytes filled so far in this process
 *   shk_debug_pool_probe         takes a block for `bytes`, downloads its first and last 32-bit word, gives it back (needs a
 *                                GPU); *block_bytes: the size of the block that was handed out.  SHK_OK, SHK_E_OOM, SHK_E_DEVICE */
int shk_debug_pool_fill(int on, uint32_t word);
uint64_t shk_debug_pool_filled_bytes(void);
int shk_debug_pool_probe(size_t bytes, uint32_t *first_word, uint32_t *last_word, size_t *block_bytes);

/* Measurement helper (bench.py): best rate in GB/s of `iters` pure streaming reads of a
 * `bytes` device buffer on the current HIP device — the achievable HBM read peak of this box, reported
 * beside the nominal 8 TB/s.  No counterpart in the reference. */
int shk_measure_stream_read(size_t bytes, int iters, double *gbs);

const char *shk_version(void);

#ifdef __cplusplus
}
#endif
#endif /* SHK_H */
