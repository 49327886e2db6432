"""GPU tests of the BGZF writer (SPEC S11a; csrc/bgzf_write_gpu.hip): the device encoder byte for byte against its host twin on
the catalogue of bgzf_write_cases.py, the JSON unescape with escape pairs on every boundary of its kernels, and
shk_get_assembly_bgzf / shk_request_assembly_bgzf on small assemblies — host writer, device writer, requested and not, one
rank and two.  Run on the MI355X box: pytest -m gpu tests/test_gpu_bgzf_write.py"""
import ctypes as C
import gzip
import json
import os
import subprocess
import sys
import tempfile

import pytest

import cases
from bgzf_write_cases import BLOCK, catalogue, check_file
from test_bgzf_write_host import host_file
from util import with_env

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "bgzf_shard_worker.py")
FIELDS = ("outfasta", "outdot", "outgfa", "outgfav2")
UNESC_CHUNK, UNESC_PER_THREAD = 2048, 8        # csrc/bgzf_write_gpu.h: bytes a workgroup / a thread of the unescape kernels takes


def device_file(lib, text, escaped=False):
    out, n = C.c_void_p(), C.c_size_t()
    if escaped:
        rc = lib.shk_device_bgzf_compress_escaped(text, len(text), C.byref(out), C.byref(n))
    else:
        ms = C.c_double()
        rc = lib.shk_device_bgzf_compress(text, len(text), C.byref(out), C.byref(n), C.byref(ms))
    if rc != 0:
        return rc
    try:
        return C.string_at(out.value, n.value)
    finally:
        lib.shk_host_free(out)


@pytest.mark.parametrize("name", [name for name, _ in catalogue()])
def test_device_files_are_the_host_files(lib, name, monkeypatch):
    text = dict(catalogue())[name]
    data = device_file(lib, text)
    assert not isinstance(data, int), data
    assert data == host_file(lib, text)
    check_file(data, text)
    if name == "three_blocks":                    # and back through the device inflater, one wave per block
        monkeypatch.setenv("SHK_GUNZIP_DEVICE_MIN", "65536")
        out, n, why = C.c_void_p(), C.c_size_t(), C.c_char_p()
        rc = lib.shk_device_gunzip(data, len(data), C.byref(out), C.byref(n), C.byref(why), None)
        assert rc == 0, (rc, why.value)
        try:
            assert C.string_at(out.value, n.value) == text
        finally:
            lib.shk_host_free(out)


def _escaped_with_pairs_at(n, pairs):
    """n bytes of JSON string content: letters, and at every offset of `pairs` the two bytes given"""
    s = bytearray((b"ACGTacgt,;: " * (n // 12 + 1))[:n])
    for at, two in pairs:
        s[at:at + len(two)] = two
    return bytes(s)


def test_escape_pairs_on_every_boundary(lib):
    """The unescape kernels take chunks of 2048 bytes, 8 consecutive bytes a thread: escape pairs with the backslash as the
    last byte of a chunk, as the first byte of a chunk, on both sides of a thread's 8 bytes, an escaped backslash in front of
    a letter n across a chunk boundary, and a run of backslashes across one.  The reference is Python's json."""
    c = UNESC_CHUNK
    pairs = [(c - 1, b"\\n"), (2 * c, b"\\n"), (3 * c - 2, b"\\t"), (7, b"\\n"), (16, b"\\\""), (23, b"\\t\\n"),
             (4 * c - 1, b"\\\\n"), (5 * c - 2, b"\\\\n"), (6 * c - 3, b"\\\\\\\\\\\"x"), (7 * c - 5, b"\\\\\\\\\\\\\\nq"),
             (40 * c + 100, b"\\n")]
    text = _escaped_with_pairs_at(40 * c + 777, pairs) + b"\\n"                  # (and a pair as the last two bytes)
    want = json.loads(b'"' + text + b'"').encode()
    assert len(want) < len(text) and b"\\n" in want                              # (an escaped backslash in front of an n is in there)
    data = device_file(lib, text, escaped=True)
    assert not isinstance(data, int), data
    assert gzip.decompress(data) == want
    assert data == host_file(lib, want)
    # every phase of a pair against the thread's 8 bytes and the chunk, one text each, the text ending at every phase too
    for phase in range(2 * UNESC_PER_THREAD):
        at = c - UNESC_PER_THREAD + phase
        text = _escaped_with_pairs_at(at + 2 + phase % 3, [(at, b"\\n")])
        data = device_file(lib, text, escaped=True)
        assert not isinstance(data, int) and gzip.decompress(data) == json.loads(b'"' + text + b'"').encode(), phase


def test_anything_else_behind_a_backslash_is_an_error(lib):
    for text in (b"ACGT\\xACGT", b"A" * 5000 + b"\\", b"\\r", b"A" * 2047 + b"\\u0041"):
        assert device_file(lib, text, escaped=True) == -6, text[-12:]
    assert gzip.decompress(device_file(lib, b"", escaped=True)) == b""


def _helper(cs, **flags):
    from sparrowhawk_amd import AssemblyHelper
    return AssemblyHelper.new(cs["k"], True, cs["min_count"], 0, 0, False, False, bool(flags.get("no_bubble_collapse")),
                              bool(flags.get("no_dead_end_removal")))


def _assembly_files(cs, flags, env, request):
    """(get_assembly() text, the four files, timings)"""
    def go():
        h = _helper(cs, **flags)
        try:
            if request is not None:
                h.request_assembly_bgzf(request)
            h.preprocess(cs["fastq"], None)
            h.assemble()
            asm = h.get_assembly()
            files = [h.get_assembly_bgzf(w) for w in range(4)]
            again = [h.get_assembly_bgzf(w) for w in (3, 0)]              # made once: the second call hands out the same file
            assert again == [files[3], files[0]]
            assert h.get_assembly() == asm
            return asm, files, h.timings()
        finally:
            h.free()
    return with_env(env, go)


ASSEMBLIES = {
    "one_contig": (lambda: cases.tip_case(), {}),
    "links": (lambda: cases.tip_case(), dict(no_dead_end_removal=True)),
    "bubble_links": (lambda: cases.bubble_case(), dict(no_bubble_collapse=True)),
    "empty": (lambda: dict(cases.tip_case(), min_count=60), {}),
}


@pytest.mark.parametrize("name", list(ASSEMBLIES))
def test_assembly_files_inflate_to_the_fields(lib, name):
    make, flags = ASSEMBLIES[name]
    cs = make()
    host_asm, host_files, t = _assembly_files(cs, flags, {"SHK_DEVICE_WRITER_MIN": None}, None)
    ref = json.loads(host_asm)
    assert (ref["ncontigs"] == 0) == (name == "empty") and (name == "one_contig") == (ref["ncontigs"] == 1)
    if "links" in name:
        assert "\nL\t" in ref["outgfa"] and "->" in ref["outdot"]
    for w, field in enumerate(FIELDS):
        assert gzip.decompress(host_files[w]) == ref[field].encode(), field
        check_file(host_files[w], ref[field].encode())
    assert t["bgzf_out_files_x1"] == 4 and "bgzf_out_from_device_x1" not in t and "device_writer_json_MB" not in t
    assert t["bgzf_out_kernels"] > 0 and "bgzf_out_d2h_host_clock" in t and t["bgzf_out_text_MB"] > 0 and t["bgzf_out_file_MB"] > 0
    # the device writer wrote the JSON; the files are made from the handle's JSON, then (requested) from the writer's buffer in HBM
    dev = {"SHK_DEVICE_WRITER_MIN": 1}
    asm1, files1, t1 = _assembly_files(cs, flags, dev, None)
    asm2, files2, t2 = _assembly_files(cs, flags, dev, 0b1111)
    asm3, files3, t3 = _assembly_files(cs, flags, dev, 0b0101)
    assert asm1 == host_asm and asm2 == host_asm and asm3 == host_asm
    assert files1 == host_files and files2 == host_files and files3 == host_files
    written_on_device = ref["ncontigs"] >= 1
    assert ("device_writer_json_MB" in t1) == written_on_device
    assert "bgzf_out_from_device_x1" not in t1 and t1["bgzf_out_files_x1"] == 4
    assert t2["bgzf_out_files_x1"] == 4 and t3["bgzf_out_files_x1"] == 4
    assert t2.get("bgzf_out_from_device_x1", 0) == (4 if written_on_device else 0)
    assert t3.get("bgzf_out_from_device_x1", 0) == (2 if written_on_device else 0)


def test_errors(lib):
    from sparrowhawk_amd import ShkError
    cs = cases.tip_case()
    h = _helper(cs)
    try:
        with pytest.raises(ShkError) as e:
            h.get_assembly_bgzf(0)
        assert e.value.code == -2
        with pytest.raises(ShkError) as e:
            h.request_assembly_bgzf(16)
        assert e.value.code == -1
        h.preprocess(cs["fastq"], None)
        with pytest.raises(ShkError) as e:
            h.get_assembly_bgzf(0)
        assert e.value.code == -2
        h.assemble()
        for which in (4, -1):
            with pytest.raises(ShkError) as e:
                h.get_assembly_bgzf(which)
            assert e.value.code == -1
        with pytest.raises(ShkError) as e:
            h.request_assembly_bgzf(1)
        assert e.value.code == -2
        assert gzip.decompress(h.get_assembly_bgzf(0)) == json.loads(h.get_assembly())["outfasta"].encode()      # (and the handle still works)
    finally:
        h.free()


# ---- sharded ------------------------------------------------------------------------------------------------------------
def _sharded_fastq():
    """a genome cut into pieces at forks: several contigs with links"""
    cs = cases.tip_case(k=31)
    return cs["fastq"] + cases.bubble_case(k=31)["fastq"]


def test_sharded_one_rank(lib):
    from sparrowhawk_amd import AssemblyHelper
    from sparrowhawk_amd.dist import LibComm, sharded_preprocess_fastq
    fq = _sharded_fastq()
    comm = LibComm(0, 1)
    try:
        seen = []
        for env, request in (({"SHK_DEVICE_WRITER_MIN": None}, None), ({"SHK_DEVICE_WRITER_MIN": 1}, None), ({"SHK_DEVICE_WRITER_MIN": 1}, 15)):
            def go():
                h = AssemblyHelper.new(31, True, 0, 0, 0, False, False, True, True)
                try:
                    if request is not None:
                        h.request_assembly_bgzf(request)
                    sharded_preprocess_fastq(h, comm, fq, split=True)
                    h.assemble()
                    return h.get_assembly(), [h.get_assembly_bgzf(w) for w in range(4)], h.timings()
                finally:
                    h.free()
            asm, files, t = with_env(env, go)
            ref = json.loads(asm)
            assert ref["ncontigs"] > 1 and "\nL\t" in ref["outgfa"]
            for w, field in enumerate(FIELDS):
                assert gzip.decompress(files[w]) == ref[field].encode(), field
            assert ("shard_writer_device_x1" in t) == ("SHK_DEVICE_WRITER_MIN" in env and env["SHK_DEVICE_WRITER_MIN"] == 1)
            assert t.get("bgzf_out_from_device_x1", 0) == (4 if request else 0)
            seen.append((asm, files))
        assert seen[0] == seen[1] == seen[2]
    finally:
        comm.free()


def test_sharded_two_ranks():
    """2 ranks on the one GPU, bytes through tests/mock_rccl: every rank's four files inflate to its get_assembly() fields, and
    the files are equal across ranks — with the host writer, and with the device writer and a request."""
    from test_dist import mock_rccl_library
    fq = _sharded_fastq()
    world = 2
    with tempfile.TemporaryDirectory() as d:
        fqp = os.path.join(d, "reads.fq")
        with open(fqp, "wb") as f:
            f.write(fq)
        cfgp, out = os.path.join(d, "cfg.json"), os.path.join(d, "res")
        with open(cfgp, "w") as f:
            json.dump({"fastq": fqp, "k": 31, "runs": [{"env": {}, "request": None}, {"env": {"SHK_DEVICE_WRITER_MIN": 1}, "request": 15}]}, f)
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
               "--master-port", "29893", WORKER, out, cfgp]
        env = dict(os.environ, OMP_NUM_THREADS="1", SHK_RCCL_LIBRARY=mock_rccl_library(), MOCK_RCCL_JITTER="0")
        pr = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, start_new_session=True)
        try:
            o, e = pr.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            import signal
            os.killpg(pr.pid, signal.SIGKILL)
            o, e = pr.communicate()
            raise AssertionError("ranks did not finish\n" + o[-2000:] + e[-2000:])
        assert pr.returncode == 0, o[-3000:] + e[-3000:]
        res = [json.load(open(f"{out}.{r}")) for r in range(world)]
    for run in range(2):
        for r in range(world):
            x = res[r][run]
            assert "error" not in x, x
            ref = json.loads(x["asm"])
            assert ref["ncontigs"] > 1
            for w, field in enumerate(FIELDS):
                assert gzip.decompress(bytes.fromhex(x["files"][w])) == ref[field].encode(), (run, r, field)
            assert x["timings"].get("bgzf_out_from_device_x1", 0) == (4 if run == 1 else 0), x["timings"]
        assert res[0][run]["files"] == res[1][run]["files"] and res[0][run]["asm"] == res[1][run]["asm"]
    assert res[0][0]["files"] == res[0][1]["files"]
