"""Wall time of the sharded preprocess from FASTQ files on the bench isolate (configs[1]: 3 333 334 reads of 150, 1.05 GB of
text) as a BGZF pair in host memory, over a one-rank communicator.  Needs a GPU.  Three ways to the same "preprocessed" handle,
alternated in one process, every call ending with the counts on the host (the device is idle):

    fastq     shk_shard_preprocess_fastq(file1, file2, split = 1)
    packed    what a caller did before: shk_pack_fastq on the inflated text of each file (the host reader, then the host parser),
              the packed arrays uploaded, shk_shard_preprocess — all of it inside the timed window
    one_gpu   shk_preprocess(file1, file2), for scale

    python tools/shard_fastq_time.py [n_reads] [reps] [warmup] [level]      one JSON line per way, then a summary line
    python tools/shard_fastq_time.py n_reads reps warmup level 1,4,16       the batch knob: `fastq` alone, the same input as it
                                                                            fits (1) and forced into about N batches through
                                                                            SHK_BATCH_BASES — one JSON line per N with the wall
                                                                            time and, per repeat, where the time and the memory go
                                                                            (verbose handles: batch_pack_kernel is a stage timer)

One rank says what the call costs, not how it scales: with N ranks each uploads and inflates 1 / N of the compressed bytes
(shard_fastq_uploaded_bytes, pinned by tests/test_gpu_shard_fastq.py), which a single GPU cannot show as a time."""
import ctypes as C
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from sparrowhawk_amd import AssemblyHelper, _lib, pack_fastq, synth
from sparrowhawk_amd.dist import LibComm, sharded_preprocess_fastq, sharded_preprocess_rccl

n_reads = int(sys.argv[1]) if len(sys.argv) > 1 else 3_333_334
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
warmup = int(sys.argv[3]) if len(sys.argv) > 3 else 2
level = int(sys.argv[4]) if len(sys.argv) > 4 else 6
forced = [int(x) for x in sys.argv[5].split(",")] if len(sys.argv) > 5 else []
K, MIN_COUNT, MIN_QUAL = 31, 5, 20
dev = torch.device("cuda", 0)
lib = _lib.load()


def make_pair():
    """the isolate's reads (seeded, drawn on the device as tools/bgzf_preprocess_time.py draws them), halved into two BGZF files"""
    from concurrent.futures import ThreadPoolExecutor
    g = torch.Generator(device=dev); g.manual_seed(0xEC02)
    genome = torch.randint(0, 4, (5_000_000,), generator=g, device=dev, dtype=torch.int32)
    parts, ar = [], torch.arange(150, device=dev)
    for r0 in range(0, n_reads, 1 << 19):
        r1 = min(n_reads, r0 + (1 << 19))
        starts = torch.randint(0, 5_000_000 - 150 + 1, (r1 - r0,), generator=g, device=dev)
        parts.append(synth.device_fastq_fixed(torch, genome[starts[:, None] + ar[None, :]]).cpu())
    fq = torch.cat(parts).numpy().tobytes()
    rec = len(fq) // n_reads                                 # fixed-width records
    half = (n_reads // 2) * rec
    out = []
    for text in (fq[:half], fq[half:]):
        per = (len(text) // 65280 // 16 + 1) * 65280         # 16 pieces of whole blocks (zlib runs without the interpreter lock)
        with ThreadPoolExecutor(16) as ex:
            z = b"".join(ex.map(lambda a: synth.bgzf_compress(text[a:a + per], level=level, eof=False), range(0, len(text), per)))
        out.append(z + synth.bgzf_compress(b""))
    return out[0], out[1], len(fq)


def host_gunzip(z):
    out, n = C.c_void_p(), C.c_size_t()
    assert lib.shk_host_gunzip(z, len(z), C.byref(out), C.byref(n), None, None) == 0
    try:
        return C.string_at(out.value, n.value)
    finally:
        lib.shk_host_free(out)


def new_handle():
    return AssemblyHelper.new(K, False, MIN_COUNT, MIN_QUAL, 0, False, False, False, False)


def way_fastq(z1, z2, comm):
    h = new_handle()
    t0 = time.perf_counter()
    sharded_preprocess_fastq(h, comm, z1, z2, split=True)
    return h, time.perf_counter() - t0


def way_packed(z1, z2, comm):
    h = new_handle()
    t0 = time.perf_counter()
    bases, seg, nb, nr = pack_fastq(host_gunzip(z1) + host_gunzip(z2), K, MIN_QUAL)
    d_bases = torch.from_numpy(bases.view(np.int32)).to(dev)
    d_seg = torch.from_numpy(seg.view(np.int32)).to(dev)
    torch.cuda.synchronize()
    sharded_preprocess_rccl(h, d_bases.data_ptr(), d_seg.data_ptr(), len(seg) - 1, nb, nr, comm)
    return h, time.perf_counter() - t0


def way_one_gpu(z1, z2, comm):
    h = new_handle()
    t0 = time.perf_counter()
    h.preprocess(z1, z2)
    return h, time.perf_counter() - t0


t0 = time.perf_counter()
z1, z2, text_bytes = make_pair()
print("# %.3f GB of text in %d reads -> %.3f + %.3f GB of BGZF at level %d (%.1f s)" % (text_bytes / 1e9, n_reads, len(z1) / 1e9, len(z2) / 1e9, level, time.perf_counter() - t0), flush=True)
comm = LibComm(0, 1)
if forced:
    KEYS = ("shard_fastq_read_host_clock", "shard_preprocess_host_clock", "shard_dedupe_kernel", "batch_pack_kernel", "batch_merge_kernel",
            "partition_kernel", "shard_pack_kernel", "shard_fastq_batches_x1", "shard_fastq_windows_x1", "shard_fastq_uploaded_bytes")
    infos = []
    for nb in forced:
        if nb > 1:
            os.environ["SHK_BATCH_BASES"] = str(text_bytes // (2 * nb) + 1)
        else:
            os.environ.pop("SHK_BATCH_BASES", None)
        wall, rows = [], []
        for rep in range(warmup + reps):
            h = AssemblyHelper.new(K, True, MIN_COUNT, MIN_QUAL, 0, False, False, False, False)
            t1 = time.perf_counter()
            sharded_preprocess_fastq(h, comm, z1, z2, split=True)
            dt = time.perf_counter() - t1
            if rep >= warmup:
                t = h.timings()
                wall.append(round(dt * 1e3, 2))
                rows.append({**{k: round(t[k], 3) for k in KEYS if k in t}, "peak_device_bytes": h.peak_device_bytes})
            info = h.get_preprocessing_info()
            h.free()
        infos.append(info)
        print(json.dumps({"way": "fastq", "asked_batches": nb, "SHK_BATCH_BASES": os.environ.get("SHK_BATCH_BASES"), "wall_ms": wall, "repeats": rows}), flush=True)
    os.environ.pop("SHK_BATCH_BASES", None)
    comm.free()
    assert all(i == infos[0] for i in infos), "the batch counts disagree"
    print(json.dumps({"summary": "same preprocessing info for every batch count", "asked_batches": forced}), flush=True)
    sys.exit(0)
ways = {"fastq": way_fastq, "packed": way_packed, "one_gpu": way_one_gpu}
ms = {w: [] for w in ways}
last, info = {}, {}
for rep in range(warmup + reps):                             # (the first handles fill the process-wide pool of device blocks)
    for name, fn in ways.items():
        h, dt = fn(z1, z2, comm)
        if rep >= warmup:
            ms[name].append(round(dt * 1e3, 2))
        last[name] = {k: v for k, v in h.timings().items() if k.startswith(("shard_fastq", "gunzip_device", "shard_preprocess_host"))}
        info[name] = h.get_preprocessing_info()
        h.free()
comm.free()
assert info["fastq"] == info["packed"] == info["one_gpu"], "the three ways disagree"
for name in ways:
    print(json.dumps({"way": name, "text_GB": text_bytes / 1e9, "file_GB": (len(z1) + len(z2)) / 1e9, "ms": ms[name], "median_ms": sorted(ms[name])[len(ms[name]) // 2],
                      "min_ms": min(ms[name]), "max_ms": max(ms[name]), "timings_of_the_last": last[name]}), flush=True)
print(json.dumps({"summary": "median ms", **{name: sorted(ms[name])[len(ms[name]) // 2] for name in ways}, "reps": reps, "warmup": warmup, "same_preprocessing_info": True}), flush=True)
