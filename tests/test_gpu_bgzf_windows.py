"""GPU tests of the windowed BGZF route (csrc/preprocess.cpp, route 2; csrc/inflate_gpu.hip: BgzfWindows and
k_last_record_start): BGZF input beyond what is inflated at once — or beyond SHK_GUNZIP_DEVICE_WINDOW, which lets small
files reach the route — is inflated, cut at record starts, parsed and counted window by window on the device.  The bytes
equal zlib's, the results those of the one-shot route, of the plain text and of the oracle; whatever goes wrong with a
window gives what the host reader gives.  Fixtures: sparrowhawk_amd.synth.bgzf_compress and the text of test_gpu_bgzf.py."""
import gzip
import struct

import numpy as np
import pytest

from sparrowhawk_amd import AssemblyHelper, ShkError, synth
from test_gpu_bgzf import EOF_BLOCK, bgzf, blocks_of, device_gunzip, fastq_text
from util import compare_all, run_oracle, sorted_table

pytestmark = pytest.mark.gpu

REC = 316                                                     # bytes of one record of fastq_text()
NONE = (1 << 64) - 1
KNOBS = ("SHK_GUNZIP_DEVICE_WINDOW", "SHK_BATCH_BASES", "SHK_GUNZIP_DEVICE", "SHK_GUNZIP_DEVICE_MIN", "SHK_HOST_PARSER")


def _with_env(monkeypatch, **env):
    """exactly these knobs; SHK_STAGE_TIMERS=0 and SHK_KEEP_STAGES=0: a handle made with verbose=False is then the quiet one
    that ships — no per-stage event timers, no synchronisation for them (a verbose handle keeps both, whatever these say)"""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("SHK_STAGE_TIMERS", "0")
    monkeypatch.setenv("SHK_KEEP_STAGES", "0")
    for k, v in env.items():
        monkeypatch.setenv("SHK_" + k, str(v))


def run(fq1, fq2=None, csize=0, min_count=3, assemble=True, verbose=True):
    h = AssemblyHelper.new(31, verbose, min_count, 20, csize, False, False, False, False)
    h.preprocess(fq1, fq2)
    if assemble:
        h.assemble()
    return h


def results(h):
    return h.get_assembly(), h.get_preprocessing_info(), h.total_instances, h.states


def outcome(*files):
    """what a user sees of a run — the error's code and message, or the outputs — and the timings of the handle"""
    h = AssemblyHelper.new(31, True, 3, 20, 0, False, False, False, False)
    try:
        h.preprocess(*files)
        h.assemble()
        return (h.get_assembly(), h.get_preprocessing_info(), h.total_instances), h.timings()
    except ShkError as e:
        return (e.code, str(e)), h.timings()


def intact_files():
    fq = fastq_text()
    part = fq[:5_000_000]
    cut = 65280 * 20
    cases = [("level %d" % lv, bgzf(lv), fq) for lv in (0, 1, 6, 9)]
    cases += [("blocks of 30000", bgzf(6, 30000), fq), ("blocks of 1000", bgzf(6, 1000), fq)]
    cases += [("no final newline", synth.bgzf_compress(part[:-1]), part[:-1]),
              ("empty blocks in mid-file", synth.bgzf_compress(part[:cut], eof=False) + EOF_BLOCK + EOF_BLOCK + synth.bgzf_compress(part[cut:]), part),
              ("no end-of-file block", synth.bgzf_compress(part, eof=False), part),
              ("two files", synth.bgzf_compress(part[:cut], level=1) + synth.bgzf_compress(part[cut:], block=30000, level=9), part),
              ("a last block of one byte", synth.bgzf_compress(part[:cut + 1]), part[:cut + 1]),
              ("a first block of one byte", synth.bgzf_compress(part[:1], eof=False) + synth.bgzf_compress(part[1:]), part),
              ("blocks of 777, stored", synth.bgzf_compress(part[:1_000_000], block=777, level=0), part[:1_000_000])]
    return cases


def test_windowed_gunzip_gives_zlibs_bytes(lib, monkeypatch):
    """1. shk_device_gunzip through the windows (100 000 bytes, 1 MiB, 5 MiB of text each) on every intact file of
    test_intact_bgzf_files_are_all_taken: 0 and exactly zlib's bytes, none declined."""
    cases = intact_files()
    for name, z, want in cases:
        assert gzip.decompress(z) == want, name
    for window in (100000, 1 << 20, 5 << 20):
        _with_env(monkeypatch, GUNZIP_DEVICE_MIN=32768, GUNZIP_DEVICE_WINDOW=window)
        for name, z, want in cases:
            rc, got, why = device_gunzip(lib, z)
            assert rc == 0, (window, name, rc, why)
            assert got == want, (window, name, len(got), len(want))


def test_windowed_gunzip_names_the_reason(lib, monkeypatch):
    """A damaged block is declined for the same reason through the windows as in one shot (one inflater serves both): block 9
    of 16 with ISIZE one less, one bit of its CRC-32 flipped, one bit in the middle of its deflate data flipped — windows of
    100 000 bytes hold one block each, so that block is decoded in mid-buffer, behind a carry.  Both ways return 1 with
    the same words; the intact file gives zlib's bytes both ways."""
    text = fastq_text()[:1_000_000]
    z = synth.bgzf_compress(text)
    bl = blocks_of(z)
    assert len(bl) == 17 and z.endswith(EOF_BLOCK)            # 16 blocks of text and the end-of-file block
    assert gzip.decompress(z) == text
    at, bsize = bl[9]
    trailer = at + bsize - 8

    def damaged(where, mask):
        b = bytearray(z)
        b[where] ^= mask
        return bytes(b)
    isize = struct.unpack_from("<I", z, trailer + 4)[0]
    less = bytearray(z)
    struct.pack_into("<I", less, trailer + 4, isize - 1)
    cases = [("ISIZE minus one", bytes(less)), ("a bit of the CRC-32", damaged(trailer + 2, 0x01)), ("a bit of the deflate data", damaged(at + bsize // 2, 0x04))]

    def both_ways(f):
        _with_env(monkeypatch, GUNZIP_DEVICE_MIN=32768)
        one_shot = device_gunzip(lib, f)
        _with_env(monkeypatch, GUNZIP_DEVICE_MIN=32768, GUNZIP_DEVICE_WINDOW=100000)
        return one_shot, device_gunzip(lib, f)
    for got in both_ways(z):
        assert got[0] == 0 and got[1] == text, got[0::2]
    for name, bad in cases:
        one_shot, windowed = both_ways(bad)
        print(name, one_shot[0::2], windowed[0::2])
        assert one_shot[0] == 1 and windowed[0] == 1, (name, one_shot[0::2], windowed[0::2])
        assert one_shot[2] and one_shot[2] == windowed[2], (name, one_shot[2], windowed[2])


def window_buffers(lib, z, text, budget):
    """the text buffers of the route's windows: the carry of the window before, then the window's text"""
    isize = np.array([struct.unpack_from("<I", z, o + b - 4)[0] for o, b in blocks_of(z)], dtype=np.uint32)
    first = np.zeros(len(isize), dtype=np.uint64)
    n = lib.shk_plan_bgzf_windows(isize.ctypes.data, len(isize), budget, first.ctypes.data, len(first))
    assert n >= 1
    ends = np.concatenate([[0], np.cumsum(isize.astype(np.int64))])
    bounds = [int(x) for x in first[:n]] + [len(isize)]
    carry = b""
    for a, b in zip(bounds, bounds[1:]):
        buf = carry + text[int(ends[a]):int(ends[b])]
        yield buf
        at = lib.shk_host_last_record_start(buf, len(buf))
        carry = buf[at:] if at != NONE else buf


def test_tail_cut_kernel_equals_the_host_rule(lib, monkeypatch):
    """3 (last item).  k_last_record_start on the window buffers of test 1's files gives what shk_host_last_record_start
    gives; so it does on text with '@' quality lines, without a boundary in its last MiB, and without any."""
    _with_env(monkeypatch)
    import ctypes as C
    fq = fastq_text()
    tails = []
    for z, text, budget in ((bgzf(6), fq, 100000), (bgzf(6, 30000), fq, 1 << 20), (synth.bgzf_compress(fq[:1_000_000], block=777, level=0), fq[:1_000_000], 100000)):
        tails += list(window_buffers(lib, z, text, budget))
    assert len(tails) > 200
    tails = tails[::3]
    rng = np.random.default_rng(20264)
    some = fq[:REC * 40]
    tails += [some[:int(e)] for e in rng.integers(1, len(some), 60)]                         # ends inside every kind of line
    tails += [some + b"A" * (3 << 20), some + b"\n".join([b"ACGT" * 20] * 40000), b"ACGT" * 100000, b"@", b"\n", b"@a\nA\n+\nI\n"]
    for t in tails:
        at = C.c_uint64(7)
        assert lib.shk_device_last_record_start(t, len(t), C.byref(at)) == 0
        assert at.value == lib.shk_host_last_record_start(t, len(t)), (len(t), t[-100:])
    assert lib.shk_host_last_record_start(tails[0], len(tails[0])) not in (0, NONE)


def halves():
    fq = fastq_text()
    half = (len(fq) // REC // 2) * REC
    return fq[:half], fq[half:]


def test_windows_through_preprocess(monkeypatch):
    """2. One BGZF file, then a pair, in bulk and in chunked mode, in windows because the text exceeds one batch
    (SHK_BATCH_BASES) or the window knob: at least eight windows, every non-empty block inflated on the device, no host
    reader; outputs, counts and progress strings equal those of the one-shot route; the oracle agrees.  (On the parent
    commit these files were read on the host and the windows key did not exist.)"""
    fq = fastq_text()
    z = bgzf(6)
    f1, f2 = halves()
    z1, z2 = synth.bgzf_compress(f1, level=1), synth.bgzf_compress(f2, block=30000, level=9)
    nb = (len(fq) + 65279) // 65280
    nb12 = (len(f1) + 65279) // 65280 + (len(f2) + 29999) // 30000
    for csize in (0, 500):
        _with_env(monkeypatch, GUNZIP_DEVICE_MIN=65536)
        one_shot, one_shot_pair = run(z, csize=csize), run(z1, z2, csize=csize)
        assert "gunzip_device_windows_x1" not in one_shot.timings() and one_shot.timings().get("gunzip_device_bgzf_blocks_x1", 0) == nb
        for knob in ({"BATCH_BASES": 150000}, {"GUNZIP_DEVICE_WINDOW": 1000000}):
            _with_env(monkeypatch, GUNZIP_DEVICE_MIN=65536, **knob)
            for files, want, blocks in (((z,), one_shot, nb), ((z1, z2), one_shot_pair, nb12)):
                h = run(*files, csize=csize)
                t = h.timings()
                print(csize, knob, len(files), {k: v for k, v in t.items() if k.startswith("gunzip")})
                assert t.get("gunzip_device_windows_x1", 0) >= 8, t
                assert t.get("gunzip_device_bgzf_blocks_x1", 0) == blocks, t
                assert t.get("gunzip_device_members_x1", 0) == len(files) and "gunzip_host_clock" not in t, t
                assert results(h) == results(want), (csize, knob, len(files))
                if csize == 0 and len(files) == 1:
                    compare_all(h, run_oracle([fq], k=31, min_count=3, min_qual=20), check_graph=False)
    # the quiet handle, which is what ships: no stage timers between the windows' kernels; the route's counters are kept all the same
    for csize in (0, 500):
        for files, blocks in (((z,), nb), ((z1, z2), nb12)):
            _with_env(monkeypatch, GUNZIP_DEVICE_MIN=65536)
            want = run(*files, csize=csize, verbose=False)
            assert "gunzip_device_windows_x1" not in want.timings()
            for knob in ({"BATCH_BASES": 150000}, {"GUNZIP_DEVICE_WINDOW": 1000000}):
                _with_env(monkeypatch, GUNZIP_DEVICE_MIN=65536, **knob)
                h = run(*files, csize=csize, verbose=False)
                t = h.timings()
                assert t.get("gunzip_device_windows_x1", 0) >= 8 and t.get("gunzip_device_bgzf_blocks_x1", 0) == blocks and "gunzip_host_clock" not in t, t
                assert "batch_pack_kernel" not in t, t           # (a stage timer of the verbose runs above: none on this handle)
                assert results(h) == results(want), (csize, knob, len(files))
    # the switches of route 1 switch this route off too
    for off in ({"GUNZIP_DEVICE": 0}, {"HOST_PARSER": 1}):
        _with_env(monkeypatch, GUNZIP_DEVICE_MIN=65536, GUNZIP_DEVICE_WINDOW=1000000, **off)
        t = run(z).timings()
        assert "gunzip_device_windows_x1" not in t and "gunzip_host_clock" in t, t


def test_carry_between_windows(lib, monkeypatch):
    """3. Windows that end in mid-record (blocks of 777 and of 30 000 bytes), quality lines that start with '@' in every
    seventh record, a last window that holds the last ten bytes of a record: the results are the plain text's."""
    fq = fastq_text()
    text = fq[:REC * 12000]                                   # 3.8 MB
    a = np.frombuffer(text, dtype=np.uint8).reshape(-1, REC).copy()
    a[::7, 15 + 150] = ord("@")
    ats = a.tobytes()
    assert ats.count(b"\n@") > len(ats) // REC
    _with_env(monkeypatch, GUNZIP_DEVICE_MIN=65536)
    plain, plain_ats = results(run(text)), results(run(ats))
    for name, z, want in (("blocks of 777", synth.bgzf_compress(text, block=777, level=0), plain),
                          ("blocks of 30000", synth.bgzf_compress(text, block=30000), plain),
                          ("'@' quality lines", synth.bgzf_compress(ats, block=30000), plain_ats),
                          ("'@' quality lines, blocks of 777", synth.bgzf_compress(ats, block=777, level=1), plain_ats)):
        _with_env(monkeypatch, GUNZIP_DEVICE_MIN=65536, GUNZIP_DEVICE_WINDOW=100000)
        h = run(z)
        t = h.timings()
        assert t.get("gunzip_device_windows_x1", 0) >= 30 and "gunzip_host_clock" not in t, (name, t)
        assert results(h) == want, name                      # (the progress strings too: the percentages are shares of the text either way)
    # a last window of ten bytes: blocks of 50 000 in pairs, then the record's end alone
    for n_rec in range(3000, 3400):
        t2 = fq[:REC * n_rec]
        main = t2[:-10]
        r = len(main) % 50000
        isize = np.array(([r] if r else []) + [50000] * (len(main) // 50000) + [10, 0], dtype=np.uint32)
        first = np.zeros(len(isize), dtype=np.uint64)
        n = lib.shk_plan_bgzf_windows(isize.ctypes.data, len(isize), 100000, first.ctypes.data, len(first))
        if int(first[n - 1]) == len(isize) - 2:
            break
    else:
        raise AssertionError("no such file")
    z = (synth.bgzf_compress(main[:r], eof=False) if r else b"") + synth.bgzf_compress(main[r:], block=50000, level=1, eof=False) + synth.bgzf_compress(t2[-10:])
    assert gzip.decompress(z) == t2
    _with_env(monkeypatch, GUNZIP_DEVICE_MIN=65536)
    want = results(run(t2))
    _with_env(monkeypatch, GUNZIP_DEVICE_MIN=65536, GUNZIP_DEVICE_WINDOW=100000)
    h = run(z)
    assert h.timings().get("gunzip_device_windows_x1", 0) == n and "gunzip_host_clock" not in h.timings(), h.timings()
    assert results(h) == want


def test_a_window_that_goes_wrong_gives_what_the_host_gives(monkeypatch):
    """4. A flipped bit in window 0 and in a later window, a wrong ISIZE, a wrong CRC-32, a blank line between two records
    of a later window: error code and message, or the outputs, are those of SHK_GUNZIP_DEVICE=0, and the later-window cases
    had their first windows inflated on the device."""
    fq = fastq_text()
    z = bgzf(6)
    bl = blocks_of(z)

    def put(at, fmt, value):
        b = bytearray(z)
        struct.pack_into(fmt, b, at, value)
        return bytes(b)

    def flip(i):
        b = bytearray(z)
        b[bl[i][0] + bl[i][1] // 2] ^= 0x04
        return bytes(b)
    t100 = bl[100][0] + bl[100][1] - 8
    mid = REC * 30000
    cases = [("a flipped bit in window 0", flip(3), False),
             ("a flipped bit in a later window", flip(100), True),
             ("a wrong ISIZE", put(t100 + 4, "<I", struct.unpack_from("<I", z, t100 + 4)[0] - 1), True),
             ("a wrong CRC-32", put(t100, "<I", struct.unpack_from("<I", z, t100)[0] ^ 0x00010000), True),
             ("a blank line between two records", synth.bgzf_compress(fq[:mid] + b"\n" + fq[mid:]), True),
             ("a record cut short in a later window", synth.bgzf_compress(fq[:mid - 100] + fq[mid:]), True)]
    for name, bad, later in cases:
        _with_env(monkeypatch, GUNZIP_DEVICE_MIN=65536, GUNZIP_DEVICE=0)
        want, t0 = outcome(bad)
        assert "gunzip_device_windows_x1" not in t0, name
        _with_env(monkeypatch, GUNZIP_DEVICE_MIN=65536, GUNZIP_DEVICE_WINDOW=1000000)
        got, t = outcome(bad)
        print(name, want if isinstance(want[0], int) else "outputs", {k: v for k, v in t.items() if k.startswith("gunzip")})
        assert got == want, name
        if later:
            assert t.get("gunzip_device_windows_x1", 0) >= 1, (name, t)
        else:
            assert "gunzip_device_windows_x1" not in t, (name, t)


def test_beyond_4_gib(monkeypatch):
    """5. 250 copies of the 18.96 MB file's blocks back to back and one end-of-file block: 4.7 GB of text, 1.3 GB
    compressed, default knobs.  Every k-mer is counted 250 times as often, in windows on the device, without the host
    reader.  (On the parent commit this file was read on the host.)"""
    _with_env(monkeypatch)
    fq = fastq_text()
    z = bgzf(6)
    assert z.endswith(EOF_BLOCK)
    big = z[:-len(EOF_BLOCK)] * 250 + EOF_BLOCK
    one = run(fq, min_count=1, assemble=False)
    h = run(big, min_count=1, assemble=False)
    del big
    t = h.timings()
    print({k: v for k, v in t.items() if k.startswith("gunzip") or k.startswith("fastq")})
    assert t.get("gunzip_device_windows_x1", 0) >= 4 and "gunzip_host_clock" not in t, t
    assert t.get("gunzip_device_bgzf_blocks_x1", 0) == 250 * (len(blocks_of(z)) - 1), t
    assert h.total_instances == 250 * one.total_instances
    k1, c1, _ = sorted_table(*one.distinct())
    k2, c2, _ = sorted_table(*h.distinct())
    assert np.array_equal(k1, k2)
    assert np.array_equal(c2.astype(np.uint64), 250 * c1.astype(np.uint64))
    hs, want = one.histo(), np.zeros(500, dtype=np.uint64)
    for i in range(500):                                      # bin i: the k-mers seen i + 1 times, the last one 500 and more
        want[min(250 * (i + 1), 500) - 1] += hs[i]
    assert np.array_equal(h.histo(), want)
