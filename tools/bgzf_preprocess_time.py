"""Wall time of shk_preprocess on the bench isolate (configs[1]: 3 333 334 reads of 150, 1.05 GB of text) as a BGZF (bgzip)
file in host memory.  Needs a GPU.

    python tools/bgzf_preprocess_time.py make FILE [n_reads] [level]     write the file (seeded; synth.bgzf_compress, 65 280-byte blocks)
    python tools/bgzf_preprocess_time.py time FILE [reps] [warmup]       one JSON line: the time of every repetition

SHK_LIB=<path to a libshk_hip.so> times another build of the library on the same file (builds are compared by running the
two alternately, one process each time); SHK_GUNZIP_DEVICE=0 is the host reader of the same build."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from sparrowhawk_amd import _lib, synth

what, path = sys.argv[1], sys.argv[2]
if what == "make":
    from concurrent.futures import ThreadPoolExecutor
    n_reads = int(sys.argv[3]) if len(sys.argv) > 3 else 3_333_334
    level = int(sys.argv[4]) if len(sys.argv) > 4 else 6
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev); g.manual_seed(0xEC02)
    genome = torch.randint(0, 4, (5_000_000,), generator=g, device=dev, dtype=torch.int32)
    parts, ar = [], torch.arange(150, device=dev)
    for r0 in range(0, n_reads, 1 << 19):
        r1 = min(n_reads, r0 + (1 << 19))
        starts = torch.randint(0, 5_000_000 - 150 + 1, (r1 - r0,), generator=g, device=dev)
        parts.append(synth.device_fastq_fixed(torch, genome[starts[:, None] + ar[None, :]]).cpu())
    fq = torch.cat(parts).numpy().tobytes()
    t0 = time.perf_counter()
    per = (len(fq) // 65280 // 16 + 1) * 65280               # 16 pieces of whole blocks (zlib runs without the interpreter lock)
    with ThreadPoolExecutor(16) as ex:
        z = b"".join(ex.map(lambda a: synth.bgzf_compress(fq[a:a + per], level=level, eof=False), range(0, len(fq), per)))
    z += synth.bgzf_compress(b"")
    open(path, "wb").write(z)
    print("%s: %.3f GB of text in %d reads -> %.3f GB of BGZF at level %d (%.1f s)" % (path, len(fq) / 1e9, n_reads, len(z) / 1e9, level, time.perf_counter() - t0), flush=True)
else:
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 7
    warmup = int(sys.argv[4]) if len(sys.argv) > 4 else 2
    if os.environ.get("SHK_LIB"):
        _lib.LIB_PATH = os.environ["SHK_LIB"]
    from sparrowhawk_amd import AssemblyHelper
    z = open(path, "rb").read()
    ms, t = [], {}
    for rep in range(warmup + reps):                          # (the first handles fill the process-wide pool of device blocks)
        h = AssemblyHelper.new(31, False, 5, 20, 0, False, False, False, False)
        t0 = time.perf_counter()
        h.preprocess(z)                                       # returns with the counts on the host: the device is idle
        dt = time.perf_counter() - t0
        if rep >= warmup:
            ms.append(round(dt * 1e3, 2))
        t, n_solid = h.timings(), h.n_solid
        h.free()
    keep = ("gunzip_device_bgzf_blocks_x1", "gunzip_device_members_x1", "gunzip_device_not_taken_x1", "gunzip_device_host_clock", "gunzip_device_h2d",
            "gunzip_device_decode", "gunzip_device_windows_resolve_crc", "gunzip_host_clock", "fastq_device_parse_pack_host_clock")
    print(json.dumps({"lib": _lib.LIB_PATH, "gunzip_device": os.environ.get("SHK_GUNZIP_DEVICE", "default"), "file_GB": len(z) / 1e9, "preprocess_ms": ms,
                      "median_ms": sorted(ms)[len(ms) // 2], "min_ms": min(ms), "max_ms": max(ms), "n_solid": n_solid,
                      "timings_of_the_last": {k: t[k] for k in keep if k in t}}), flush=True)
