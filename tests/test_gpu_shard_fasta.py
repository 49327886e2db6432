"""GPU tests of the sharded preprocess from FASTA files (shk_shard_preprocess_fasta): the grid-wide header search
(k_fasta_header_search) against the host rule at the edges of its lane groups, waves and workgroups; every rank's slice of
plain, gzip and BGZF input through shk_device_pack_fasta_slice; the whole call over a one-rank communicator against
shk_preprocess_fasta and the oracle, in one batch and in many; and worlds of 2 and 3 ranks over the stand-in transport
(tests/mock_rccl)."""
import ctypes as C
import gzip
import json
import os
import signal
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import fasta_cases as fa
import test_gpu_shard_fastq as sq
from sparrowhawk_amd import AssemblyHelper, ShkError, _lib
from sparrowhawk_amd.helper import pack_fasta
from test_gpu_fasta import genome_collection, reads_fasta
from util import compare_all, run_oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "shard_fasta_worker.py")
NONE = (1 << 64) - 1
KNOBS = ("SHK_HOST_PARSER", "SHK_BATCH_BASES", "SHK_GUNZIP_DEVICE", "SHK_GUNZIP_DEVICE_WINDOW")
_cache = {}


@pytest.fixture(autouse=True)
def knobs(monkeypatch):
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("SHK_GUNZIP_DEVICE_MIN", "4096")
    monkeypatch.setenv("SHK_FASTA_DEVICE_MIN", "0")


def reads(seed=5, genome=30000, coverage=12):
    """reads of a genome as FASTA, wrapped at 70"""
    key = ("reads", seed, genome, coverage)
    if key not in _cache:
        _cache[key] = reads_fasta(genome, coverage, seed, err=0.005)
    return _cache[key]


def collection():
    """the three genomes of tests/test_gpu_fasta.py as one text: records of 40 kbp"""
    if "collection" not in _cache:
        _cache["collection"] = [fa.fa(b"isolate%d some words" % j, s, 60) for j, s in enumerate(genome_collection())]
    return _cache["collection"]


def halves(text):
    cut = text.index(b"\n>", len(text) // 2) + 1
    return text[:cut], text[cut:]


# ---- 1. the kernels against the host functions -------------------------------------------------------------------------
def device_first(lib, t, frm):
    at = C.c_uint64(0)
    assert lib.shk_device_first_fasta_record_start(t, len(t), frm, C.byref(at)) == 0
    return int(at.value)


def device_last(lib, t):
    at = C.c_uint64(0)
    assert lib.shk_device_last_fasta_record_start(t, len(t), C.byref(at)) == 0
    return int(at.value)


def host_first(lib, t, frm):
    return int(lib.shk_host_first_fasta_record_start(t, len(t), frm))


def host_last(lib, t):
    return int(lib.shk_host_last_fasta_record_start(t, len(t)))


def test_the_header_search_equals_the_host_functions(lib):
    rng = np.random.default_rng(777)
    rec = lambda i, n, w=60: fa.fa(b"r%d" % i, fa.seq_of(rng, n), w)      # noqa: E731
    small = b"".join(rec(i, int(n)) for i, n in enumerate(rng.integers(0, 400, 40)))
    texts = {
        "a header at byte 0": small,
        "blank lines in front": b"\n\r\n" + small,
        "CRLF": small.replace(b"\n", b"\r\n"),
        "> not at a line start": b">a x>y\nAC>GT\nA\r>C\n" + b"ACGT>ACGT\n" * 300 + b">z\nAC\n",
        "no header at all": b"ACGT\n" * 1000,
        "only a header as the last byte": b"ACGT\n" * 500 + b">",
        "> as the last byte, behind no newline": b">a\n" + b"ACGT" * 500 + b">",
        "one byte": b">",
        "empty": b"",
    }
    # texts of every length mod 16 (the entry uploads a text n % 16 bytes behind a 16-byte boundary: every alignment of the
    # head and tail groups)
    for m in range(16):
        texts["length %d mod 16" % m] = (small * 2)[:4096 + 37 * 16 + m]
    for name, t in texts.items():
        starts = [i for i in range(len(t)) if t[i] == 62 and (i == 0 or t[i - 1] == 10)]
        froms = [0, 1, 15, 16, 17, 63, 64, 1023, 1024, 4095, 4096, max(len(t) - 1, 0), len(t)] + [int(x) for x in rng.integers(0, len(t) + 1, 20)]
        froms += [s + d for s in starts[:3] + starts[-2:] for d in (0, 1)]      # on a header, and one past it: the next one
        for frm in froms:
            got = device_first(lib, t, frm)
            assert got == host_first(lib, t, frm), (name, frm)
            assert got == min((s for s in starts if s >= frm), default=NONE), (name, frm)
        assert device_last(lib, t) == host_last(lib, t) == (starts[-1] if starts else NONE), name
        for n in [int(x) for x in rng.integers(0, len(t) + 1, 6)]:          # (the last start of some prefixes)
            assert device_last(lib, t[:n]) == host_last(lib, t[:n]), (name, n)
    # '\n' as the last byte and '>' as the first byte of a 16-byte lane group, of a wave's 1024 bytes, of a workgroup's 4096:
    # the groups lie at 16-byte aligned addresses, so the first group begins (n % 16 + from) % 16 bytes in front of `from`
    for a in (0, 5, 15):
        for frm in (0, 3, 16, 1000):
            for edge in (16, 1024, 4096, 8192):
                for shift in (-1, 0, 1):
                    at = frm - ((a + frm) % 16) + edge + shift
                    if at < max(frm, 1):
                        continue
                    t = bytearray(b"ACGT" * 3000)
                    del t[len(t) - ((len(t) - a) % 16):]
                    assert len(t) % 16 == a
                    t[at - 1:at + 1] = b"\n>"
                    t[at + 40:at + 42] = b"\n>"                              # (a later one must not be taken for the first)
                    t = bytes(t)
                    assert device_first(lib, t, frm) == host_first(lib, t, frm) == at, (a, frm, edge, shift)
                    assert device_last(lib, t) == host_last(lib, t) == at + 41, (a, frm, edge, shift)
                    assert device_last(lib, t[:at + 41]) == host_last(lib, t[:at + 41]) == at, (a, frm, edge, shift)
                    # from one past it: the next header; from behind both: none
                    assert device_first(lib, t, at + 1) == at + 41 and device_first(lib, t, at + 42) == NONE
    # headers only beyond the first reach of 1 MiB: the host widens the limit and asks again
    far = b"N" * ((1 << 20) + 1000) + b"\n" + small[:5000]
    assert device_first(lib, far, 5) == host_first(lib, far, 5) == (1 << 20) + 1001
    assert device_first(lib, far[:1 << 20], 5) == NONE
    # the last start far in front of the end: headers only in the first bytes of a 3 MiB text
    t = b">a\nAC\n>b\n" + b"ACGT" * (3 << 18)
    assert device_last(lib, t) == host_last(lib, t) == 6
    assert device_last(lib, t + b"\n>") == len(t) + 1                       # a header as the last byte
    for frm in [int(x) for x in rng.integers(0, len(t), 20)]:
        assert device_first(lib, t, frm) == host_first(lib, t, frm) == (NONE if frm > 6 else 6 if frm else 0), frm


# ---- 2. every rank's slice, without a communicator -----------------------------------------------------------------------
def ref_segments(t1, k, t2=None):
    words, seg, n_reads, _ = fa.ref_pack_fasta(t1, k, t2)
    return sorted(sq.segments(words, seg)), n_reads


def device_slice(lib, f1, f2, k, rank, world):
    """(rc, segments, n_reads, uploaded_bytes, route or message)"""
    out = _lib.ShkPacked()
    up, route = C.c_uint64(0), C.c_char_p()
    rc = lib.shk_device_pack_fasta_slice(f1, len(f1), f2, len(f2) if f2 is not None else 0, k, rank, world, C.byref(out), C.byref(up), C.byref(route))
    what = (route.value or b"").decode()
    if rc != 0:
        return rc, None, 0, int(up.value), what
    try:
        bases = np.ctypeslib.as_array(out.bases, shape=((out.n_bases >> 4) + 2,)).copy()
        seg = np.ctypeslib.as_array(out.seg_off, shape=(out.n_seg + 1,)).copy()
        assert int(seg[-1]) == out.n_bases and int(seg[0]) == 0
        return 0, sq.segments(bases, seg), int(out.n_reads), int(up.value), what
    finally:
        lib.shk_packed_free(C.byref(out))


@pytest.mark.parametrize("data", ["reads", "genomes"])
@pytest.mark.parametrize("kind", ["text", "gz", "bgzf", "pair"])
def test_the_slices_of_all_ranks_hold_every_record_once(lib, kind, data):
    k = 31
    if data == "reads":
        text = reads()
        a, b = halves(text)
    else:
        genomes = collection()
        text, a, b = b"".join(genomes), genomes[0] + genomes[1], genomes[2]
    if kind == "text":
        files, ok_routes, plain = (text, None), {"text_slice"}, (text, None)
    elif kind == "gz":
        files, ok_routes, plain = (gzip.compress(text, compresslevel=6), None), {"member_whole", "host"}, (text, None)      # (the member inflater is speculative: it may decline)
    elif kind == "bgzf":
        files, ok_routes, plain = (sq.bgzf_write(text, 4096), None), {"bgzf_slice"}, (text, None)
        assert len(sq.blocks_of(files[0])) >= 25
    else:
        files, ok_routes, plain = (sq.bgzf_write(a[:-1], 4096), b), {"bgzf_slice+text_slice"}, (a[:-1], b)      # (file 1 ends without a newline)
    want, want_reads = ref_segments(plain[0], k, plain[1])
    assert want_reads == text.count(b">") and len(want) >= 3
    size = len(files[0]) + (len(files[1]) if files[1] else 0)
    for world in (1, 2, 3, 5):
        segs, n_reads, ups, routes = [], 0, [], []
        for r in range(world):
            rc, s, nr, up, route = device_slice(lib, files[0], files[1], k, r, world)
            assert rc == 0, (r, world, rc, route)
            segs += s; n_reads += nr; ups.append(up); routes.append(route)
        print(kind, data, "world", world, "routes", routes, "uploaded", ups, "of", size)
        assert set(routes) <= ok_routes and len(set(routes)) == 1, (world, routes)
        assert n_reads == want_reads, (world, n_reads)
        assert sorted(segs) == want, world
        if kind == "bgzf" and data == "reads" and world == 3:
            assert all(u < 0.6 * size for u in ups), (ups, size)           # a rank uploads its run and a few blocks, not the file
    if data == "genomes" and kind == "text":
        # records of 40 kbp: at world 5 some slices are empty
        assert [device_slice(lib, text, None, k, r, 5)[2] for r in range(5)].count(0) >= 2


# ---- 3. refusals -----------------------------------------------------------------------------------------------------
def test_a_line_in_front_of_the_first_header_of_file_2_is_refused_in_slice_0(lib):
    text = reads()
    rc, _, _, _, msg = device_slice(lib, text, b"ACGT\n" + text, 31, 0, 2)
    assert rc == -3 and "FASTA" in msg, (rc, msg)
    assert device_slice(lib, text, b"ACGT\n" + text, 31, 1, 2)[0] == 0
    rc, _, _, _, msg = device_slice(lib, b"ACGT\n" + text, None, 31, 0, 2)
    assert rc == -3 and "FASTA" in msg, (rc, msg)


def test_an_oversized_share_is_a_parameter_error(lib, monkeypatch):
    monkeypatch.setenv("SHK_BATCH_BASES", "100000")
    text = reads()
    assert len(text) > 300000
    rc, _, _, _, msg = device_slice(lib, text, None, 31, 0, 2)
    assert rc == -1 and "exceeds one batch" in msg, (rc, msg)
    assert device_slice(lib, text, None, 31, 0, 8)[0] == 0            # (an eighth of the text fits)


# ---- 4. world 1 over the real communicator ---------------------------------------------------------------------------
def run(comm, f1, f2, k, split, min_count=3, correct=True, sharded=True):
    from sparrowhawk_amd.dist import sharded_preprocess_fasta
    h = AssemblyHelper.new(k, True, min_count, 20, 0, False, False, not correct, not correct)
    if sharded:
        sharded_preprocess_fasta(h, comm, f1, f2, split=bool(split))
    else:
        h.preprocess_fasta(f1, f2)
    h.assemble()
    return h


@pytest.mark.parametrize("k", [31, 63])
def test_world_1_equals_preprocess_fasta_and_the_oracle(k):
    """shk_shard_preprocess_fasta with a one-rank RCCL communicator: text, .gz, BGZF and a pair, split 0 and 1."""
    from sparrowhawk_amd.dist import LibComm, sharded_preprocess_fasta
    text = reads(seed=20 + k, genome=40000, coverage=14)
    a, b = halves(text)
    inputs = {"text": (text, None, "shard_fasta_text_slice_x1"), "gz": (gzip.compress(text), None, None),
              "bgzf": (sq.bgzf_write(text, 4096), None, "shard_fasta_bgzf_slice_x1"), "pair": (sq.bgzf_write(a, 4096), gzip.compress(b), None)}
    oracle = run_oracle([fa.fastq_twin(text)], k=k, min_count=3, min_qual=20)
    comm = LibComm(0, 1)
    try:
        for name, (f1, f2, marker) in inputs.items():
            ref = run(comm, f1, f2, k, 0, sharded=False)
            for split in (1, 0):
                h = run(comm, f1, f2, k, split)
                t = h.timings()
                print(name, "split", split, {x: v for x, v in t.items() if x.startswith("shard_fasta")})
                assert h.get_preprocessing_info() == ref.get_preprocessing_info(), (name, split)
                assert h.get_assembly() == ref.get_assembly(), (name, split)
                assert t["shard_fasta_uploaded_bytes"] > 0 and "shard_exchange_host_clock" in t
                assert t["shard_fasta_batches_x1"] == (2 if f2 is not None else 1), (name, t)
                if marker:
                    assert t.get(marker, 0) == 1, (name, t)
                assert h.states[:2] == ref.states[:2] and h.states[-1] == "assembly:end"
                loops = [s for s in h.states if ":loop:" in s and not s.endswith(":end")]
                assert loops and loops[-1].endswith(":%d:100" % text.count(b">")), loops
                if split:
                    compare_all(h, oracle, check_graph=False)
                h.free()
            ref.free()
        # the state rules of shk_shard_preprocess: a used handle is refused
        h = AssemblyHelper.new(k, False, 3, 20, 0, False, False, False, False)
        sharded_preprocess_fasta(h, comm, text)
        with pytest.raises(ShkError) as ei:
            sharded_preprocess_fasta(h, comm, text)
        assert ei.value.code == -2
        h.free()
    finally:
        comm.free()


def test_world_1_a_collection_of_genomes_gives_its_compacted_de_bruijn_graph():
    """min_count = 0 and both corrections off, as the README's example: records of 40 kbp through the BGZF route"""
    from sparrowhawk_amd.dist import LibComm
    k = 31
    whole = b"".join(collection())
    comm = LibComm(0, 1)
    try:
        ref = run(comm, whole, None, k, 0, min_count=0, correct=False, sharded=False)
        h = run(comm, sq.bgzf_write(whole, 4096), None, k, 1, min_count=0, correct=False)
        assert h.timings().get("shard_fasta_bgzf_slice_x1", 0) == 1, h.timings()
        assert h.get_preprocessing_info() == ref.get_preprocessing_info() and h.get_assembly() == ref.get_assembly()
        compare_all(h, run_oracle([fa.fastq_twin(whole)], k=k, min_count=0, min_qual=20, no_bubble_collapse=True, no_dead_end_removal=True), check_graph=False)
        h.free(); ref.free()
    finally:
        comm.free()


# ---- 5. batches ------------------------------------------------------------------------------------------------------
def test_world_1_in_batches(monkeypatch):
    from sparrowhawk_amd.dist import LibComm, sharded_preprocess_fasta
    k = 31
    text = reads()
    a, b = halves(text)
    inputs = {"text": (text, None), "gz": (gzip.compress(text), None), "bgzf": (sq.bgzf_write(text, 4096), None),
              "pair": (sq.bgzf_write(a[:-1], 4096), b)}
    comm = LibComm(0, 1)
    try:
        ref = run(comm, text, None, k, 1)                           # one batch
        assert ref.timings()["shard_fasta_batches_x1"] == 1
        want = (ref.get_preprocessing_info(), ref.get_assembly())
        monkeypatch.setenv("SHK_BATCH_BASES", "20000")
        monkeypatch.setenv("SHK_GUNZIP_DEVICE_WINDOW", "65536")
        cut = text.index(b"\n>", len(text) // 2) + 1
        long_record = text[:cut] + fa.fa(b"long", b"ACGT" * 7500, 70) + text[cut:]
        for host in (False, True):
            if host:
                monkeypatch.setenv("SHK_HOST_PARSER", "1")
            for name, (f1, f2) in inputs.items():
                h = run(comm, f1, f2, k, 1)
                t = h.timings()
                print(name, "host parser" if host else "", {x: v for x, v in t.items() if x.startswith("shard_fasta")})
                assert t["shard_fasta_batches_x1"] > 10, (name, t)
                assert (h.get_preprocessing_info(), h.get_assembly()) == want, (name, host)
                loops = [s for s in h.states if ":loop:" in s and not s.endswith(":end")]
                # (one string per batch; one more where the text the rank expected of a file was an estimate that the batches did not reach)
                assert 0 <= len(loops) - t["shard_fasta_batches_x1"] <= 1 and loops[-1].endswith(":%d:100" % text.count(b">")), loops[-3:]
                if host:
                    assert t.get("shard_fasta_host_x1", 0) == (2 if f2 is not None else 1), (name, t)
                h.free()
            # a record of 30 000 bases in the middle: never split
            for name, f1 in (("text", long_record), ("gz", gzip.compress(long_record)), ("bgzf", sq.bgzf_write(long_record, 4096))):
                h = AssemblyHelper.new(k, False, 3, 20, 0, False, False, False, False)
                with pytest.raises(ShkError) as ei:
                    sharded_preprocess_fasta(h, comm, f1)
                assert ei.value.code == -1 and "exceeds one batch" in str(ei.value) and "a single FASTA record of 30" in str(ei.value), (name, str(ei.value))
                h.free()
        ref.free()
    finally:
        comm.free()


# ---- 6. worlds of 2 and 3 over the stand-in transport ----------------------------------------------------------------
def launch(nproc, args, port, timeout):
    """as tests/test_gpu_shard_fastq.py launches its workers: a process group of its own, ended as a whole at the time limit"""
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
    """Case A: split = 1, the same BGZF pair on every rank.  Case B: split = 0, a file per rank, rank 1 without one.  Case C: as A
    under a small SHK_BATCH_BASES, so that the ranks take different numbers of batches.  Case D: split = 0 with sequence in front
    of the first header in rank 1's file, which every rank must leave together: SHK_E_PARSE with the host packer's message there,
    "another rank failed during reading" elsewhere."""
    from test_dist import mock_rccl_library
    assert world <= 3
    k = 31
    text = reads(seed=30 + world)
    a, b = halves(text)
    junk = b"ACGT\n" + b
    with pytest.raises(ShkError) as ei:
        pack_fasta(junk, k)
    packer_message = str(ei.value)
    assert "SHK_E_PARSE" in packer_message and "FASTA" in packer_message
    monkeypatch.setenv("SHK_RCCL_LIBRARY", mock_rccl_library())
    with tempfile.TemporaryDirectory() as d:
        def put(name, data):
            p = os.path.join(d, name)
            open(p, "wb").write(data)
            return p
        pa, pb = put("a.fa.gz", sq.bgzf_write(a, 4096)), put("b.fa.gz", sq.bgzf_write(b, 4096))
        ta, tb, tjunk = put("a.fa", a), put("b.fa", b), put("junk.fa", junk)
        own = [[ta, None], None, [tb, None]][:world] if world == 3 else [[put("ab.fa.gz", gzip.compress(text)), None], None]
        bad = [[ta, None], [tjunk, None], [tb, None]][:world]
        cases = [{"files": [[pa, pb]] * world, "split": 1},
                 {"files": own, "split": 0},
                 {"files": [[pa, pb]] * world, "split": 1, "env": {"SHK_BATCH_BASES": 30000, "SHK_GUNZIP_DEVICE_WINDOW": 65536}},
                 {"files": bad, "split": 0}]
        for cs in cases:
            cs.update(k=k, min_count=3)
        cfgp = put("cfg.json", json.dumps({"cases": cases}).encode())
        out = os.path.join(d, "res")
        launch(world, [out, cfgp], 29950 + world, timeout=240)
        res = [json.load(open(f"{out}.{r}")) for r in range(world)]
    o = run_oracle([fa.fastq_twin(text)], k=k, min_count=3, min_qual=20)
    o.assemble()
    for r in range(world):
        for case in (0, 1, 2):
            x = res[r][case]
            assert "error" not in x, (r, case, x)
            assert x["pre"] == o.preprocessing_json() and x["asm"] == o.assembly_json(), (r, case)
        assert res[r][0]["timings"].get("shard_fasta_bgzf_slice_x1", 0) == 2, res[r][0]["timings"]
        assert res[r][2]["timings"].get("shard_fasta_batches_x1", 0) >= 2, res[r][2]["timings"]
        x = res[r][3]
        assert "error" in x, (r, x)
        if r == 1:
            assert x["code"] == -3 and x["error"] == packer_message, x
        else:
            assert "another rank failed during reading" in x["error"], x
    print("case C batches per rank:", [res[r][2]["timings"].get("shard_fasta_batches_x1") for r in range(world)])
