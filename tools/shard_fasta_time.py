"""Wall time of the sharded preprocess from FASTA files on a generated collection of genomes (isolates of one core genome with
SNPs, one record each, a few megabytes a record, several hundred megabytes of text) as one BGZF file in host memory, over a
one-rank communicator.  Needs a GPU.  Ways to the same "preprocessed" handle, alternated in one process:

    shard_fasta           shk_shard_preprocess_fasta(file, split = 1), the share in one batch
    shard_fasta_batches   the same under a small SHK_BATCH_BASES (about N batches: windows of the rank's run, cut at headers)
    one_gpu               shk_preprocess_fasta(file), for scale

and, separately, the header search (csrc/inflate_gpu.hip: k_fasta_header_search) on one text that holds a single record of 16 MiB,
forwards (from byte 1 to the header behind the record) and backwards (from the end to the header at byte 0).  The entry points
that run the kernel alone (shk_device_first_fasta_record_start / shk_device_last_fasta_record_start) upload the text first, so
the figure is a difference: the call on the 16 MiB record minus the call on the same text where the search ends in its first
reach (from = 0: the header at byte 0; a header as the last byte).  The one-wave FASTQ kernel (k_first_record_start) walks the
same text for comparison.

    python tools/shard_fasta_time.py [n_genomes] [genome_bp] [reps] [warmup] [n_batches]      one JSON line per way, then the kernel lines

One rank says what the call costs, not how it scales: with N ranks each uploads and inflates 1 / N of the compressed bytes
(shard_fasta_uploaded_bytes, pinned by tests/test_gpu_shard_fasta.py), which a single GPU cannot show as a time."""
import ctypes as C
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch  # noqa: F401  (torch's HIP runtime first)
from sparrowhawk_amd import AssemblyHelper, _lib, synth
from sparrowhawk_amd.dist import LibComm, sharded_preprocess_fasta

n_genomes = int(sys.argv[1]) if len(sys.argv) > 1 else 64
genome_bp = int(sys.argv[2]) if len(sys.argv) > 2 else 4_000_000
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
warmup = int(sys.argv[4]) if len(sys.argv) > 4 else 1
n_batches = int(sys.argv[5]) if len(sys.argv) > 5 else 8
K, WIDTH = 31, 80
lib = _lib.load()


def make_collection():
    """isolates of one core genome, about one SNP in 1000 bases each, one record per isolate, lines of WIDTH; BGZF at level 1"""
    from concurrent.futures import ThreadPoolExecutor
    core = synth.random_genome(genome_bp // WIDTH * WIDTH, 4040)
    rng = np.random.default_rng(4041)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    recs = []
    for j in range(n_genomes):
        g = core.copy()
        at = rng.integers(0, len(g), len(g) // 1000)
        g[at] = (g[at] + 1 + rng.integers(0, 3, len(at))) & 3
        lines = np.empty((len(g) // WIDTH, WIDTH + 1), dtype=np.uint8)
        lines[:, :WIDTH] = letters[g].reshape(-1, WIDTH)
        lines[:, WIDTH] = 10
        recs.append(b">isolate%d generated\n" % j + lines.tobytes())
    text = b"".join(recs)
    per = (len(text) // 65280 // 16 + 1) * 65280             # 16 pieces of whole blocks (zlib runs without the interpreter lock)
    with ThreadPoolExecutor(16) as ex:
        z = b"".join(ex.map(lambda a: synth.bgzf_compress(text[a:a + per], level=1, eof=False), range(0, len(text), per)))
    return z + synth.bgzf_compress(b""), len(text), len(recs[0])


def timed(fn):
    h = AssemblyHelper.new(K, False, 0, 20, 0, False, False, True, True)
    t0 = time.perf_counter()
    fn(h)
    return h, time.perf_counter() - t0


t0 = time.perf_counter()
z, text_bytes, record_bytes = make_collection()
print("# %.3f GB of text in %d records of %.2f MB -> %.3f GB of BGZF (%.1f s)" % (text_bytes / 1e9, n_genomes, record_bytes / 1e6, len(z) / 1e9, time.perf_counter() - t0), flush=True)
comm = LibComm(0, 1)
small = str(text_bytes // n_batches + 1)
ways = {"shard_fasta": (None, lambda h: sharded_preprocess_fasta(h, comm, z, split=True)),
        "shard_fasta_batches": (small, lambda h: sharded_preprocess_fasta(h, comm, z, split=True)),
        "one_gpu": (None, lambda h: h.preprocess_fasta(z))}
ms, last, info = {w: [] for w in ways}, {}, {}
for rep in range(warmup + reps):                             # (the first handles fill the process-wide pool of device blocks)
    for name, (batch_bases, fn) in ways.items():
        if batch_bases:
            os.environ["SHK_BATCH_BASES"] = batch_bases
        h, dt = timed(fn)
        os.environ.pop("SHK_BATCH_BASES", None)
        if rep >= warmup:
            ms[name].append(round(dt * 1e3, 2))
        last[name] = {k: round(v, 3) for k, v in h.timings().items() if k.startswith(("shard_fasta", "fasta_", "gunzip_device", "shard_preprocess_host"))}
        info[name] = h.get_preprocessing_info()
        h.free()
comm.free()
assert info["shard_fasta"] == info["shard_fasta_batches"] == info["one_gpu"], "the ways disagree"
for name, (batch_bases, _) in ways.items():
    print(json.dumps({"way": name, "SHK_BATCH_BASES": batch_bases, "text_GB": text_bytes / 1e9, "file_GB": len(z) / 1e9, "ms": ms[name],
                      "median_ms": sorted(ms[name])[len(ms[name]) // 2], "timings_of_the_last": last[name]}), flush=True)
print(json.dumps({"summary": "median ms", **{name: sorted(ms[name])[len(ms[name]) // 2] for name in ways}, "reps": reps, "warmup": warmup,
                  "same_preprocessing_info": True}), flush=True)

# ---- the header search across one record of 16 MiB
body = (b"ACGT" * (WIDTH // 4) + b"\n") * ((16 << 20) // (WIDTH + 1))
one = b">one record\n" + body


def call_ms(fn, n=5):
    out = []
    for _ in range(n + 1):
        at = C.c_uint64(0)
        t1 = time.perf_counter()
        assert fn(C.byref(at)) == 0
        out.append((time.perf_counter() - t1) * 1e3)
    return round(sorted(out[1:])[n // 2], 3), int(at.value)


fwd = one + b">"                                              # the next header: the last byte
far, at_far = call_ms(lambda at: lib.shk_device_first_fasta_record_start(fwd, len(fwd), 1, at))
near, at_near = call_ms(lambda at: lib.shk_device_first_fasta_record_start(fwd, len(fwd), 0, at))
assert at_far == len(fwd) - 1 and at_near == 0
print(json.dumps({"kernel": "k_fasta_header_search<first>", "record_MiB": len(one) / 2 ** 20, "call_across_the_record_ms": far, "call_that_ends_at_once_ms": near,
                  "search_ms": round(far - near, 3)}), flush=True)
far, at_far = call_ms(lambda at: lib.shk_device_last_fasta_record_start(one, len(one), at))
near, at_near = call_ms(lambda at: lib.shk_device_last_fasta_record_start(fwd, len(fwd), at))
assert at_far == 0 and at_near == len(fwd) - 1
print(json.dumps({"kernel": "k_fasta_header_search<last>", "record_MiB": len(one) / 2 ** 20, "call_across_the_record_ms": far, "call_that_ends_at_once_ms": near,
                  "search_ms": round(far - near, 3)}), flush=True)
walk, at_walk = call_ms(lambda at: lib.shk_device_first_record_start(fwd, len(fwd), 1, at), n=1)
print(json.dumps({"kernel": "k_first_record_start (one wave, the FASTQ rule, the same text: no start in it)", "call_ms": walk, "found": at_walk != (1 << 64) - 1}), flush=True)
