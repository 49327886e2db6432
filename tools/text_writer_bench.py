"""The two writers from contig text alone, side by side: shk_host_assembly_json (the host writer on the host's cores) and
shk_device_assembly_json (csrc/writer_text_gpu.h; the call also makes a pipeline object and uploads the text, so it is an
upper bound of what the sharded assembly pays, whose text is in HBM already).  Contigs: a random text cut into pieces of
40-60 bases (the configs[4] share averages 50), every piece on whichever strand it falls — half of them get turned.
Usage: python tools/text_writer_bench.py [n_contigs ...] [--runs R]     (needs a GPU)"""
import argparse, ctypes as C, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
try:
    import torch  # noqa: F401  (torch's HIP runtime first, as the tests do)
except Exception:
    pass
from sparrowhawk_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument("sizes", nargs="*", type=int, default=[2000, 5000, 20000, 100000, 1000000, 4000000])
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--k", type=int, default=31)
a = ap.parse_args()
lib = _lib.load()


def call(device, seqs, off, kc, n):
    t0 = time.perf_counter()
    if device:
        why = C.c_char_p()
        p = lib.shk_device_assembly_json(seqs, off.ctypes.data, kc.ctypes.data, n, a.k, C.byref(why))
        assert p, why.value
    else:
        p = lib.shk_host_assembly_json(seqs, off.ctypes.data, kc.ctypes.data, n, a.k)
        assert p
    dt = time.perf_counter() - t0
    text = C.string_at(p)
    lib.shk_host_free(p)
    return dt, text


for n in a.sizes:
    rng = np.random.default_rng(n)
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum(rng.integers(40, 61, n))
    seqs = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, int(off[-1]))].tobytes()
    kc = rng.integers(1, 5000, n).astype(np.uint64)
    call(True, seqs, off, kc, n)                               # (first device call of a size: the block pool grows)
    host, dev, same = [], [], True
    for _ in range(a.runs):                                     # the two alternating
        th, xh = call(False, seqs, off, kc, n)
        td, xd = call(True, seqs, off, kc, n)
        host.append(th); dev.append(td); same &= xh == xd
    print("%9d contigs, %6.1f MB of JSON: host %8.2f ms (%s)  device entry %8.2f ms (%s)  same bytes: %s" % (
        n, len(xh) / 1e6, 1e3 * statistics.median(host), " ".join("%.2f" % (1e3 * t) for t in host),
        1e3 * statistics.median(dev), " ".join("%.2f" % (1e3 * t) for t in dev), same), flush=True)
