"""GPU tests of the sharded preprocess from FASTQ files (shk_shard_preprocess_fastq): the device kernel that finds where a
slice begins (k_first_record_start) against the host rule, every rank's slice of plain, gzip and BGZF input through
shk_device_pack_fastq_slice (the routes of split = 1 without a communicator), the whole call over a one-rank communicator
against shk_preprocess and the oracle, and worlds of 2 and 3 ranks over the stand-in transport (tests/mock_rccl)."""
import ctypes as C
import gzip
import json
import os
import signal
import struct
import subprocess
import sys
import tempfile
import zlib

import numpy as np
import pytest

from sparrowhawk_amd import AssemblyHelper, ShkError, _lib, pack_fastq, synth
from util import compare_all, run_oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "shard_fastq_worker.py")
NONE = (1 << 64) - 1
_cache = {}


# ---- a small BGZF writer (SAM specification 4.1; tests/test_gpu_bgzf.py reads the format) --------------------------------
def bgzf_block(chunk, level=6):
    """one block: a gzip member with the 'BC' extra subfield that holds its size - 1, raw deflate, CRC-32, ISIZE"""
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    d = c.compress(chunk) + c.flush()
    bsize = 18 + len(d) + 8
    assert bsize <= 65536
    return struct.pack("<4BI2BH2BHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, bsize - 1) + d + struct.pack("<II", zlib.crc32(chunk), len(chunk))


def bgzf_write(data, payload=4096, level=6, eof=True):
    """`data` in blocks of `payload` bytes of text, the empty end-of-file block behind them"""
    out = [bgzf_block(data[i:i + payload], level) for i in range(0, len(data), payload)]
    return b"".join(out) + (bgzf_block(b"") if eof else b"")


def blocks_of(z):
    out, p = [], 0
    while p < len(z):
        bsize = struct.unpack_from("<H", z, p + 16)[0] + 1
        out.append((p, bsize))
        p += bsize
    return out


def dataset(seed=7, genome=30000, n_reads=4000, read_len=150):
    key = (seed, genome, n_reads, read_len)
    if key not in _cache:
        g = synth.random_genome(genome, seed)
        codes, quals = synth.sample_reads(g, n_reads, read_len, seed + 1, err=0.01)
        _cache[key] = bytes(synth.to_fastq(codes, quals))
    return _cache[key]


def halves(fq):
    """the reads of a text as the two files of a pair"""
    cut = fq.find(b"\n@r", len(fq) // 2) + 1
    return fq[:cut], fq[cut:]


# ---- 1. the kernel against the host rule ------------------------------------------------------------------------------
def device_first(lib, t, frm):
    at = C.c_uint64(0)
    assert lib.shk_device_first_record_start(t, len(t), frm, C.byref(at)) == 0
    return int(at.value)


def host_first(lib, t, frm):
    return int(lib.shk_host_first_record_start(t, len(t), frm))


def test_device_first_record_start_equals_the_host_function(lib):
    rng = np.random.default_rng(4242)

    def rec(i, ln, q0=b"I"):
        seq = bytes(rng.choice(list(b"ACGT"), ln).tolist())
        return b"@r%d\n" % i + seq + b"\n+\n" + q0 + b"I" * (ln - 1) + b"\n"
    texts = {
        "reads of 100-150": dataset(seed=9, n_reads=2000)[:60000],
        "lines longer than 64 and 128 bytes": b"".join(rec(i, [70, 130, 200, 64, 65, 128, 129, 63][i % 8], [b"@", b"+", b"I"][i % 3]) for i in range(60)),
        "short lines, qualities that begin with @ and +": b"".join(rec(i, 1 + i % 5, [b"@", b"+"][i % 2]) for i in range(80)),
        # the first start lies more than two steps of 64 bytes ahead: a long line that is no record in front of the records
        "a start far ahead": b"x" * 300 + b"\n" + b"y" * 10 + b"\n" + b"".join(rec(i, 90) for i in range(5)),
        "no start at all": b"ACGT\n" * 100,
        "CRLF": dataset(seed=9, n_reads=2000)[:20000].replace(b"\n", b"\r\n"),
    }
    for name, t in texts.items():
        froms = [0, 63, 64, 65, 127, 128] + [int(x) for x in rng.integers(0, len(t), 20)] + [len(t) - 1, len(t)]
        for frm in froms:
            assert device_first(lib, t, frm) == host_first(lib, t, frm), (name, frm)
    # a cut text: the start at or behind `from` exists in the whole text but is undecided in the part — on both sides
    t = texts["lines longer than 64 and 128 bytes"]
    last = t.rfind(b"\n@r") + 1
    plus = t.find(b"\n+\n", last) + 1
    for n in (plus, plus - 1, last + 3, plus + 1, plus + 2):
        cut = t[:n]
        got = device_first(lib, cut, last)
        assert got == host_first(lib, cut, last), n
        assert got == (NONE if n <= plus else last), (n, got)
    assert device_first(lib, b"", 0) == NONE
    # (far ahead: beyond the first reach of 1 MiB the host widens the limit and asks again)
    far = b"N" * ((1 << 20) + 1000) + b"\n" + texts["reads of 100-150"][:5000]
    assert device_first(lib, far, 5) == host_first(lib, far, 5) == (1 << 20) + 1001


# ---- 2. every rank's slice, without a communicator -------------------------------------------------------------------
def segments(bases, seg):
    """the segment strings of a packed batch"""
    codes = ((np.asarray(bases, dtype=np.uint32)[:, None] >> (2 * np.arange(16, dtype=np.uint32))) & 3).astype(np.uint8).reshape(-1)
    text = np.frombuffer(b"ACGT", dtype=np.uint8)[codes].tobytes()
    return [text[int(a):int(b)] for a, b in zip(seg, seg[1:])]


def host_pack(fq, k, min_qual=20):
    bases, seg, nb, nr = pack_fastq(fq, k, min_qual)
    return sorted(segments(bases, seg)), nr


def device_slice(lib, f1, f2, k, rank, world, min_qual=20):
    """(rc, segments, n_reads, uploaded_bytes, route or message)"""
    out = _lib.ShkPacked()
    up, route = C.c_uint64(0), C.c_char_p()
    rc = lib.shk_device_pack_fastq_slice(f1, len(f1), f2, len(f2) if f2 is not None else 0, k, min_qual, rank, world,
                                         C.byref(out), C.byref(up), C.byref(route))
    what = (route.value or b"").decode()
    if rc != 0:
        return rc, None, 0, int(up.value), what
    try:
        bases = np.ctypeslib.as_array(out.bases, shape=((out.n_bases >> 4) + 2,)).copy()
        seg = np.ctypeslib.as_array(out.seg_off, shape=(out.n_seg + 1,)).copy()
        assert int(seg[-1]) == out.n_bases and int(seg[0]) == 0
        return 0, segments(bases, seg), int(out.n_reads), int(up.value), what
    finally:
        lib.shk_packed_free(C.byref(out))


def all_ranks(lib, f1, f2, k, world):
    segs, reads, ups, routes = [], 0, [], []
    for r in range(world):
        rc, s, nr, up, route = device_slice(lib, f1, f2, k, r, world)
        assert rc == 0, (r, world, rc, route)
        segs += s; reads += nr; ups.append(up); routes.append(route)
    return sorted(segs), reads, ups, routes


@pytest.mark.parametrize("kind", ["text", "gz", "bgzf", "bgzf_pair"])
def test_the_slices_of_all_ranks_hold_every_read_once(lib, monkeypatch, kind):
    monkeypatch.setenv("SHK_GUNZIP_DEVICE_MIN", "4096")
    k = 31
    fq = dataset()
    want, want_reads = host_pack(fq, k)
    assert 2000 <= want_reads <= 6000
    if kind == "text":
        files, ok_routes = (fq, None), {"text_slice"}
    elif kind == "gz":
        files, ok_routes = (gzip.compress(fq, compresslevel=6), None), {"member_whole", "host"}      # (the member inflater is speculative: it may decline)
    elif kind == "bgzf":
        files, ok_routes = (bgzf_write(fq, 4096), None), {"bgzf_slice"}
        assert len(blocks_of(files[0])) >= 30
    else:
        a, b = halves(fq)
        assert a.count(b"\n") % 4 == 0 and b.startswith(b"@r")
        files, ok_routes = (bgzf_write(a[:-1], 4096), bgzf_write(b, 3000, level=1)), {"bgzf_slice"}      # (file 1 ends without a newline)
    size = len(files[0]) + (len(files[1]) if files[1] else 0)
    for world in (1, 2, 3, 5):
        got, reads, ups, routes = all_ranks(lib, files[0], files[1], k, world)
        print(kind, "world", world, "routes", routes, "uploaded", ups, "of", size)
        assert set(routes) <= ok_routes and len(set(routes)) == 1, (world, routes)
        assert reads == want_reads, (world, reads)
        assert got == want, world
        if kind.startswith("bgzf") and world == 3:
            assert all(u < 0.6 * size for u in ups), (ups, size)       # a rank uploads its run and a few blocks, not the file


def test_a_damaged_bgzf_block_goes_through_the_fallback_or_fails_as_preprocess_does(lib, monkeypatch):
    monkeypatch.setenv("SHK_GUNZIP_DEVICE_MIN", "4096")
    k, world = 31, 3
    fq = dataset()
    z = bgzf_write(fq, 4096)
    bl = blocks_of(z)
    i = len(bl) // 2
    crc_at = bl[i][0] + bl[i][1] - 8
    flipped_crc = bytearray(z); flipped_crc[crc_at] ^= 0x01
    flipped_data = bytearray(z); flipped_data[bl[i][0] + bl[i][1] // 2] ^= 0x04
    for name, bad in (("CRC-32 flipped", bytes(flipped_crc)), ("a bit of the stream flipped", bytes(flipped_data))):
        # what shk_preprocess does with the file
        h = AssemblyHelper.new(k, False, 3, 20, 0, False, False, False, False)
        try:
            h.preprocess(bad)
            whole = 0
        except ShkError as e:
            whole = e.code
        h.free()
        results = [device_slice(lib, bad, None, k, r, world) for r in range(world)]
        print(name, "shk_preprocess:", whole, "ranks:", [(rc, route) for rc, _, _, _, route in results])
        if whole == 0:                       # the host reader takes the file: so does every rank, through the fallback
            out, n = C.c_void_p(), C.c_size_t()
            assert lib.shk_host_gunzip(bad, len(bad), C.byref(out), C.byref(n), None, None) == 0
            text = C.string_at(out.value, n.value)
            lib.shk_host_free(out)
            assert all(rc == 0 for rc, *_ in results)
            assert "host" in [route for *_, route in results]
            assert sorted(s for _, segs, *_ in results for s in segs) == host_pack(text, k)[0]
        else:                                # SHK_E_PARSE, on the ranks that have the block in view; the others hold their slices
            assert whole == -3
            assert all(rc in (0, -3) for rc, *_ in results) and -3 in [rc for rc, *_ in results]
            want = host_pack(fq, k)[0]
            for rc, segs, *_ in results:
                if rc == 0:
                    assert set(segs) <= set(want)


def test_an_oversized_share_is_a_parameter_error(lib, monkeypatch):
    monkeypatch.setenv("SHK_BATCH_BASES", "100000")
    fq = dataset()
    rc, _, _, _, msg = device_slice(lib, fq, None, 31, 0, 2)
    assert rc == -1 and "exceeds one batch" in msg, (rc, msg)
    assert device_slice(lib, fq, None, 31, 0, 8)[0] == 0            # (an eighth of the text fits)


# ---- 3. world 1 over the real communicator ---------------------------------------------------------------------------
@pytest.mark.parametrize("k", [31, 63])
def test_world_1_equals_preprocess_and_the_oracle(monkeypatch, k):
    """shk_shard_preprocess_fastq with a one-rank RCCL communicator (set up as tests/test_dist.py:
    test_rccl_inside_the_library_world_1 does): text, .gz, BGZF and a pair, split 0 and 1."""
    monkeypatch.setenv("SHK_GUNZIP_DEVICE_MIN", "4096")
    from sparrowhawk_amd.dist import LibComm, sharded_preprocess_fastq
    fq = dataset(seed=20 + k, genome=40000, n_reads=6000)
    a, b = halves(fq)
    inputs = {"text": (fq, None, "shard_fastq_text_slice_x1"), "gz": (gzip.compress(fq), None, None),
              "bgzf": (bgzf_write(fq, 4096), None, "shard_fastq_bgzf_slice_x1"), "pair": (bgzf_write(a, 4096), gzip.compress(b), None)}
    comm = LibComm(0, 1)
    try:
        for name, (f1, f2, marker) in inputs.items():
            ref = AssemblyHelper.new(k, True, 3, 20, 0, False, False, False, False)
            ref.preprocess(f1, f2)
            ref.assemble()
            for split in (1, 0):
                h = AssemblyHelper.new(k, True, 3, 20, 0, False, False, False, False)
                sharded_preprocess_fastq(h, comm, f1, f2, split=bool(split))
                h.assemble()
                t = h.timings()
                print(name, "split", split, {x: v for x, v in t.items() if x.startswith("shard_fastq")})
                assert h.get_preprocessing_info() == ref.get_preprocessing_info(), (name, split)
                assert h.get_assembly() == ref.get_assembly(), (name, split)
                assert t["shard_fastq_uploaded_bytes"] > 0 and "shard_exchange_host_clock" in t
                if marker:
                    assert t.get(marker, 0) == 1, (name, t)
                assert h.states[:2] == ref.states[:2] and h.states[-1] == "assembly:end"
                if split:
                    compare_all(h, run_oracle([fq], k=k, min_count=3, min_qual=20), check_graph=False)
                h.free()
            ref.free()
        # the state rules of shk_shard_preprocess: a used handle is refused
        h = AssemblyHelper.new(k, False, 3, 20, 0, False, False, False, False)
        sharded_preprocess_fastq(h, comm, fq)
        with pytest.raises(ShkError) as ei:
            sharded_preprocess_fastq(h, comm, fq)
        assert ei.value.code == -2
        h.free()
    finally:
        comm.free()


# ---- 4. worlds of 2 and 3 over the stand-in transport ----------------------------------------------------------------
def launch(nproc, args, port, timeout):
    """as tests/test_dist.py launches its workers: a process group of its own, ended as a whole at the time limit"""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), WORKER] + args
    env = dict(os.environ, OMP_NUM_THREADS="1")
    pr = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, start_new_session=True)
    try:
        out, errs = pr.communicate(timeout=timeout)
    except subprocess.TimeoutExpired:
        os.killpg(pr.pid, signal.SIGKILL)
        out, errs = pr.communicate()
        raise AssertionError(f"ranks did not finish within {timeout} s\n" + out[-2000:] + errs[-2000:])
    assert pr.returncode == 0, out[-3000:] + errs[-3000:]


@pytest.mark.parametrize("world", [2, 3])
def test_several_ranks_over_the_stand_in_transport(monkeypatch, world):
    """Case A: split = 1, the same BGZF pair on every rank.  Case B: split = 0, a file per rank, rank 1 without one.  Then
    the failures, which every rank must leave together: rank 1's file cut in the middle of a record (SHK_E_PARSE with the
    host parser's message there, "another rank failed during reading" elsewhere), and SHK_FAULT_INJECT=read on rank 0."""
    from test_dist import mock_rccl_library
    assert world <= 3
    k = 31
    fq = dataset(seed=30 + world, genome=30000, n_reads=4000)
    a, b = halves(fq)
    cut = a[:a.rfind(b"\n@r") + 1 + 40]                      # ends inside a sequence line
    with pytest.raises(ShkError) as ei:
        pack_fastq(cut, k, 20)
    parser_message = str(ei.value)
    assert "SHK_E_PARSE" in parser_message
    monkeypatch.setenv("SHK_RCCL_LIBRARY", mock_rccl_library())
    monkeypatch.setenv("SHK_GUNZIP_DEVICE_MIN", "4096")
    with tempfile.TemporaryDirectory() as d:
        def put(name, data):
            p = os.path.join(d, name)
            open(p, "wb").write(data)
            return p
        pa, pb = put("a.fq.gz", bgzf_write(a, 4096)), put("b.fq.gz", bgzf_write(b, 4096))
        ta, tb, tcut = put("a.fq", a), put("b.fq", b), put("cut.fq", cut)
        own = [[ta, None], None, [tb, None]][:world] if world == 3 else [[put("ab.fq.gz", gzip.compress(fq)), None], None]
        bad = [[ta, None], [tcut, None], [tb, None]][:world]
        cases = [{"files": [[pa, pb]] * world, "split": 1},
                 {"files": own, "split": 0},
                 {"files": bad, "split": 0},
                 {"files": [[pa, pb]] * world, "split": 1, "inject": {"rank": 0, "step": "read"}}]
        for cs in cases:
            cs.update(k=k, min_count=3)
        cfgp = put("cfg.json", json.dumps({"cases": cases}).encode())
        out = os.path.join(d, "res")
        launch(world, [out, cfgp], 29930 + world, timeout=240)
        res = [json.load(open(f"{out}.{r}")) for r in range(world)]
    o = run_oracle([fq], k=k, min_count=3, min_qual=20)
    o.assemble()
    for r in range(world):
        for case in (0, 1):
            x = res[r][case]
            assert "error" not in x, (r, case, x)
            assert x["pre"] == o.preprocessing_json() and x["asm"] == o.assembly_json(), (r, case)
        assert res[r][0]["timings"].get("shard_fastq_bgzf_slice_x1", 0) == 2, res[r][0]["timings"]
        x = res[r][2]
        assert "error" in x, (r, x)
        if r == 1:
            assert x["code"] == -3 and x["error"] == parser_message, x
        else:
            assert "another rank failed during reading" in x["error"], x
        x = res[r][3]
        assert "error" in x, (r, x)
        assert ("injected fault" if r == 0 else "another rank failed during reading") in x["error"], x
