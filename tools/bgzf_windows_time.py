"""Times shk_preprocess on a BGZF file beyond 4 GiB of text (250 copies of the 18.96 MB fixture's blocks, one end-of-file
block: 4.7 GB of text, 1.3 GB compressed) through the windowed device route at several window sizes and through the host
reader (SHK_GUNZIP_DEVICE=0: the path such a file took before the route existed).  Median of RUNS calls after one warm-up
each, new handle per call; then shk_peak_device_bytes for the fixture itself, one-shot against 1 MiB windows.
    python tools/bgzf_windows_time.py [RUNS]          (RUNS = 0: one call at the default and nothing else, to be traced)"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
try:
    import torch  # noqa: F401  (one HIP runtime for both)
except Exception:
    pass
from sparrowhawk_amd import AssemblyHelper, synth  # noqa: E402

RUNS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
KNOBS = ("SHK_GUNZIP_DEVICE", "SHK_GUNZIP_DEVICE_WINDOW", "SHK_GUNZIP_DEVICE_MIN")


def fixture():
    g = synth.random_genome(200000, 15)
    codes, quals = synth.sample_reads(g, 60000, 150, 16, err=0.01)
    return bytes(synth.to_fastq_fixed(codes, quals))


def once(z, env):
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(env)
    h = AssemblyHelper.new(31, False, 3, 20, 0, False, False, False, False)
    t0 = time.perf_counter()
    h.preprocess(z)
    dt = time.perf_counter() - t0
    out = dt, h.total_instances, h.peak_device_bytes, h.timings()
    h.free()
    return out


def main():
    fq = fixture()
    z = synth.bgzf_compress(fq)
    eof = synth.bgzf_compress(b"")
    big = z[:-len(eof)] * 250 + eof
    print("file: %.3f GB compressed, %.3f GB of text" % (len(big) / 1e9, 250 * len(fq) / 1e9), flush=True)
    legs = [("host reader (SHK_GUNZIP_DEVICE=0)", {"SHK_GUNZIP_DEVICE": "0"}),
            ("windows of 256 MiB", {"SHK_GUNZIP_DEVICE_WINDOW": str(256 << 20)}),
            ("windows of 1 GiB (default)", {}),
            ("windows of 2 GiB", {"SHK_GUNZIP_DEVICE_WINDOW": str(2 << 30)})]
    if RUNS == 0:                                             # one call at the default, for a kernel trace of a run of its own
        dt, inst, peak, t = once(big, {})
        print("one call, windows of 1 GiB: %.3f s, %s windows" % (dt, t.get("gunzip_device_windows_x1")), flush=True)
        return
    want = None
    for name, env in legs:
        once(big, env)
        ts = []
        for _ in range(RUNS):
            dt, inst, peak, t = once(big, env)
            ts.append(dt)
            want = inst if want is None else want
            assert inst == want, (name, inst, want)
        print("%-36s median %.3f s (min %.3f, max %.3f) of %d; peak device bytes %.2f GB; windows %s" %
              (name, statistics.median(ts), min(ts), max(ts), RUNS, peak / 1e9, t.get("gunzip_device_windows_x1")), flush=True)
    for name, env in (("fixture, one-shot", {"SHK_GUNZIP_DEVICE_MIN": "65536"}),
                      ("fixture, windows of 1 MiB", {"SHK_GUNZIP_DEVICE_MIN": "65536", "SHK_GUNZIP_DEVICE_WINDOW": str(1 << 20)})):
        once(z, env)
        dt, inst, peak, t = once(z, env)
        print("%-36s peak device bytes %.1f MB (%.1f ms)" % (name, peak / 1e6, dt * 1e3), flush=True)


if __name__ == "__main__":
    main()
