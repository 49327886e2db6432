"""Rates of the two FASTA packers (needs a GPU).

  python tools/fasta_pack_rate.py [--mb 200] [--repeats 3] [--sizes 1,4,16,64,200]

Packs a FASTA text of about --mb MB made from synth genomes on 60-character lines, and the same bases as 150-bp reads, with
gpu_pack_fasta (GB/s of text from the timers of shk_preprocess_fasta, every figure over the repeats: fasta_h2d_text the upload,
fasta_device_kernels the kernels, fasta_device_parse_pack_host_clock the packer's whole call; no download is in them; a text
that is one single record is among them) and with shk_pack_fasta on the host, and times shk_preprocess_fasta end to end by each packer at the
sizes given.  One warm-up run per figure, then --repeats runs: min / median / max are printed, one JSON line at the end.
The default of SHK_FASTA_DEVICE_MIN is the smallest size at which the device route is not slower than the host route by more
than the spread of the repeats (profiles/fasta/README.txt)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
try:
    import torch  # noqa: F401  (one HIP runtime for both, as bench.py does)
except Exception:
    pass
from sparrowhawk_amd import AssemblyHelper, _lib, synth  # noqa: E402

_ASCII = np.frombuffer(b"ACGT", dtype=np.uint8)


def genomes_text(n_bytes, width=60, genome=4_000_000):
    parts, size, i = [], 0, 0
    while size < n_bytes:
        n = min(genome, max(1000, (n_bytes - size) * width // (width + 1)))
        s = _ASCII[synth.random_genome(n, 100 + i)]
        pad = (-n) % width
        lines = np.concatenate((s, np.full(pad, ord("A"), np.uint8))).reshape(-1, width)
        body = np.concatenate((lines, np.full((len(lines), 1), 10, np.uint8)), axis=1).tobytes()
        parts.append(b">genome%d\n" % i + body)
        size += len(parts[-1]); i += 1
    return b"".join(parts)


def reads_text(n_bytes, read_len=150, width=60):
    g = synth.random_genome(4_000_000, 7)
    per = 8 + read_len + (read_len + width - 1) // width
    n = max(1, n_bytes // per)
    starts = np.random.default_rng(8).integers(0, len(g) - read_len, n)
    s = _ASCII[g[starts[:, None] + np.arange(read_len)[None, :]]]
    rows = [np.frombuffer(b">r%06d\n" % 0, np.uint8)[None, :].repeat(n, 0)]
    for a in range(0, read_len, width):
        rows += [s[:, a:a + width], np.full((n, 1), 10, np.uint8)]
    return np.concatenate(rows, axis=1).tobytes()


def stats(xs):
    xs = sorted(xs)
    return {"min": xs[0], "median": xs[len(xs) // 2], "max": xs[-1]}


def timed(fn, repeats):
    fn()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return stats(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sizes", default="1,4,16,64,200")
    ap.add_argument("--k", type=int, default=31)
    a = ap.parse_args()
    L = _lib.load()
    res = {"k": a.k, "repeats": a.repeats}

    def host_pack(text):
        out, err = _lib.ShkPacked(), C.c_char_p()
        assert L.shk_pack_fasta(text, len(text), a.k, C.byref(out), C.byref(err)) == 0
        L.shk_packed_free(C.byref(out))

    def preprocess(text, host):
        os.environ["SHK_HOST_PARSER" if host else "SHK_FASTA_DEVICE_MIN"] = "1" if host else "0"
        try:
            h = AssemblyHelper.new(a.k, False, 0, 20, 0, False, False, False, False)
            h.preprocess_fasta(text)
            t = h.timings()
            h.free()
            return t
        finally:
            os.environ.pop("SHK_HOST_PARSER", None); os.environ.pop("SHK_FASTA_DEVICE_MIN", None)

    def device_figures(text):
        """upload, kernels and the packer's whole call (upload + kernels + its host waits; no download), each over the repeats"""
        preprocess(text, False)
        ts = [preprocess(text, False) for _ in range(a.repeats)]
        return {key: stats([t[key] for t in ts]) for key in ("fasta_h2d_text", "fasta_device_kernels", "fasta_device_parse_pack_host_clock")}

    one_genome = lambda n: genomes_text(n, genome=1 << 40)      # noqa: E731  (a single record: one run, all pieces from one thread)
    for name, make in (("genomes", genomes_text), ("one_genome", one_genome), ("reads_150", reads_text)):
        text = make(a.mb << 20)
        gb = len(text) / 1e9
        d = device_figures(text)
        hst = timed(lambda: host_pack(text), max(1, a.repeats - 1))
        res[name] = {"bytes": len(text), "device_ms": d, "host_pack_ms": hst,
                     "device_pack_GBps": gb / (d["fasta_device_parse_pack_host_clock"]["median"] / 1e3),
                     "device_kernels_GBps": gb / (d["fasta_device_kernels"]["median"] / 1e3),
                     "upload_GBps": gb / (d["fasta_h2d_text"]["median"] / 1e3),
                     "host_GBps": gb / (hst["median"] / 1e3)}
        print(name, json.dumps(res[name]), flush=True)
    whole = genomes_text(max(int(s) for s in a.sizes.split(",")) << 20)
    res["preprocess_fasta_ms"] = {}
    for mb in (int(s) for s in a.sizes.split(",")):
        cut = whole.rfind(b"\n", 0, mb << 20) + 1
        text = whole[:cut]
        row = {"bytes": len(text)}
        for host in (False, True):
            row["host" if host else "device"] = timed(lambda: preprocess(text, host), a.repeats)
        res["preprocess_fasta_ms"][str(mb)] = row
        print("preprocess_fasta", mb, "MB", json.dumps(row), flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
