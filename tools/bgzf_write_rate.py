"""The outputs as BGZF files (shk_get_assembly_bgzf; SPEC S11a) on one MI355X, for two assemblies:
    isolate      the bench isolate (BASELINE configs[1]: 5 Mbp, 100x 150 bp reads, k=31): one contig, the host writer's JSON
    fragmented   configs[2]'s reads with their errors left in (k=51, 1 % substitutions) at 10x instead of 100x, min_count 1: at
                 100x that assembly is one contig too; thinned out it breaks at every stretch the reads cover once or not at
                 all and lies above SHK_DEVICE_WRITER_MIN (asserted), so the device writer writes its JSON
Per output it prints one JSON line: text and file bytes beside zlib at levels 1 and 6 on the same text (timed on one host
core), and bgzf_out_kernels / bgzf_out_d2h_host_clock / the wall time of the call, unrequested (made from the handle's JSON at
the first shk_get_assembly_bgzf) and requested (made inside shk_assemble; from HBM where the device writer wrote the JSON),
the median of --runs handles after one warm-up handle.  A last line per assembly has the writer's own download
(device_writer_d2h_host_clock, device_writer_json_MB, or for the host writer collapse_d2h_contigs_host_clock) from handles
that ask for no file.  --writer-only prints only that line and touches nothing this tool's commit added, so the same file
runs against the parent commit's library.
Usage: python tools/bgzf_write_rate.py [--runs R] [--only isolate|fragmented] [--writer-only]     (needs a GPU)"""
import argparse
import gzip
import json
import os
import statistics
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("SHK_STAGE_TIMERS", "1")          # bgzf_out_kernels is an event timer
import torch  # noqa: E402  (torch's HIP runtime first, as bench.py does)

import bench  # noqa: E402
from sparrowhawk_amd import AssemblyHelper, synth  # noqa: E402

FIELDS = ("outfasta", "outdot", "outgfa", "outgfav2")
ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--only", default=None)
ap.add_argument("--writer-only", action="store_true")
ap.add_argument("--genome", type=int, default=5_000_000)
a = ap.parse_args()
dev = torch.device("cuda", 0)
n_reads = (a.genome * 100 + 149) // 150


def median(xs):
    return round(statistics.median(xs), 4)


def assembled(k, reads, request=None):
    d_bases, d_seg, n_seg, n_bases, min_count = reads
    h = AssemblyHelper.new(k, False, min_count, 20, 0, False, False, False, False)
    if request is not None:
        h.request_assembly_bgzf(request)
    h.preprocess_packed_device(d_bases.data_ptr(), d_seg.data_ptr(), n_seg, n_bases, n_seg)
    h.assemble()
    return h


def measure(name, k, reads):
    # ---- the writer's own download, from handles that ask for nothing
    rows = []
    for i in range(a.runs + 1):
        h = assembled(k, reads)
        t = h.timings()
        if i == 0:
            ncontigs = json.loads(h.get_assembly())["ncontigs"]
            assert name != "fragmented" or (ncontigs >= 20000 and "device_writer_json_MB" in t), (ncontigs, sorted(t))
        h.free()
        if i:
            rows.append(t)
    keys = ("device_writer_d2h_host_clock", "device_writer_json_MB", "device_writer_kernels", "collapse_d2h_contigs_host_clock", "outputs_host_clock")
    line = {"assembly": name, "ncontigs": ncontigs, "what": "the writer's own download, no file asked for", "runs": a.runs}
    line.update({key: median([t[key] for t in rows]) for key in keys if key in rows[0]})
    print(json.dumps(line), flush=True)
    if a.writer_only:
        return
    # ---- unrequested: the file is made at the first call, from the handle's JSON on the host
    per = {w: {"kernels": [], "d2h": [], "wall": []} for w in range(4)}
    texts, files = None, None
    for i in range(a.runs + 1):
        h = assembled(k, reads)
        if i == 0:
            ref = json.loads(h.get_assembly())
            texts = [ref[f].encode() for f in FIELDS]
        before = h.timings()
        got = []
        for w in range(4):
            t0 = time.perf_counter()
            got.append(h.get_assembly_bgzf(w))
            wall = 1e3 * (time.perf_counter() - t0)
            now = h.timings()
            if i:
                per[w]["kernels"].append(now["bgzf_out_kernels"] - before.get("bgzf_out_kernels", 0.0))
                per[w]["d2h"].append(now["bgzf_out_d2h_host_clock"] - before.get("bgzf_out_d2h_host_clock", 0.0))
                per[w]["wall"].append(wall)
            before = now
        assert files is None or got == files, "the files differ between two handles"
        files = got
        h.free()
    # ---- requested: one handle per output, the file made inside assemble
    req = {w: {"kernels": [], "d2h": [], "from_device": 0} for w in range(4)}
    for w in range(4):
        for i in range(a.runs + 1):
            h = assembled(k, reads, request=1 << w)
            asked = h.timings()
            assert h.get_assembly_bgzf(w) == files[w], "the requested file differs from the unrequested one"
            t = h.timings()                                  # (the host writer's JSON: the file is made at the call, requested or not)
            assert ("bgzf_out_files_x1" in asked) == ("device_writer_json_MB" in asked)
            h.free()
            if i:
                req[w]["kernels"].append(t["bgzf_out_kernels"]); req[w]["d2h"].append(t["bgzf_out_d2h_host_clock"])
                req[w]["from_device"] = int(t.get("bgzf_out_from_device_x1", 0))
    for w, field in enumerate(FIELDS):
        text = texts[w]
        assert gzip.decompress(files[w]) == text
        z = {}
        for level in (1, 6):
            t0 = time.perf_counter()
            z[level] = len(zlib.compress(text, level))
            z["ms%d" % level] = round(1e3 * (time.perf_counter() - t0), 2)
        print(json.dumps({"assembly": name, "ncontigs": ncontigs, "output": field, "text_bytes": len(text), "file_bytes": len(files[w]),
                          "bits_per_byte": round(8 * len(files[w]) / max(1, len(text)), 4),
                          "zlib1_bytes": z[1], "zlib1_host_ms": z["ms1"], "zlib6_bytes": z[6], "zlib6_host_ms": z["ms6"],
                          "unrequested": {"bgzf_out_kernels": median(per[w]["kernels"]), "bgzf_out_d2h_host_clock": median(per[w]["d2h"]),
                                          "call_wall_ms": median(per[w]["wall"])},
                          "requested": {"bgzf_out_kernels": median(req[w]["kernels"]), "bgzf_out_d2h_host_clock": median(req[w]["d2h"]),
                                        "from_device": req[w]["from_device"]}, "runs": a.runs}), flush=True)


if a.only in (None, "isolate"):
    d_bases, d_seg, n, n_bases, _ = bench.make_reads_on_device(torch, dev, a.genome, 100, 150, 0xEC02)
    measure("isolate", 31, (d_bases, d_seg, n, n_bases, 5))
    del d_bases, d_seg
if a.only in (None, "fragmented"):
    dr = synth.device_reads(torch, dev, a.genome, n_reads // 10, 150, 51, 0xEC03, err=0.01, mask_errors=False)
    measure("fragmented", 51, (dr.words, dr.seg_off, dr.n_seg, dr.n_bases, 1))
