"""GPU tests of the sharded preprocess with SEVERAL batches per rank: shk_shard_preprocess_fastq on shares beyond one batch
(a BGZF run window by window, text and gzip members piece by piece) and shk_shard_preprocess_batches on packed reads.  Small
shapes on purpose: SHK_BATCH_BASES = 100000 makes the 600 k bases of 4000 reads six batches and more.  Every comparison is
exact: a share cut into batches gives the bytes shk_preprocess gives on the same files, and the oracle's."""
import gzip
import json
import os
import tempfile

import numpy as np
import pytest

from sparrowhawk_amd import AssemblyHelper, ShkError, pack_fastq, synth
from test_gpu_shard_fastq import bgzf_write, dataset, halves, launch
from util import compare_all, run_oracle

pytestmark = pytest.mark.gpu

BATCH = 100000
_refs = {}


def small_batches(monkeypatch, batch=BATCH):
    monkeypatch.setenv("SHK_BATCH_BASES", str(batch))
    monkeypatch.setenv("SHK_GUNZIP_DEVICE_MIN", "4096")


def reference(files, k, **kw):
    """(preprocessing info, assembly) of shk_preprocess on the same files, computed once per input"""
    key = (hash(files[0]), hash(files[1]), k, tuple(sorted(kw.items())))
    if key not in _refs:
        ref = AssemblyHelper.new(k, False, kw.get("min_count", 3), kw.get("min_qual", 20), 0, False, False, False, False)
        ref.preprocess(files[0], files[1])
        ref.assemble()
        _refs[key] = (ref.get_preprocessing_info(), ref.get_assembly())
        ref.free()
    return _refs[key]


def sharded(comm, files, k, split=True, do_bloom=False, min_count=3, min_qual=20):
    from sparrowhawk_amd.dist import sharded_preprocess_fastq
    h = AssemblyHelper.new(k, True, min_count, min_qual, 0, do_bloom, False, False, False)
    sharded_preprocess_fastq(h, comm, files[0], files[1], split=split)
    return h


def inputs_of(fq):
    a, b = halves(fq)
    return {"text": ((fq, None), {"shard_fastq_text_slice_x1": 1}),
            "gz": ((gzip.compress(fq, compresslevel=6), None), {}),       # (the member inflater is speculative: member_whole or host)
            "bgzf": ((bgzf_write(fq, 4096), None), {"shard_fastq_bgzf_slice_x1": 1}),
            "pair bgzf + gz": ((bgzf_write(a, 4096), gzip.compress(b)), {"shard_fastq_bgzf_slice_x1": 1}),
            "pair of texts": ((a, b), {"shard_fastq_text_slice_x1": 2})}


def packed_bases(fq, k):
    return int(pack_fastq(fq, k, 20)[2])


# ---- 1. world 1 over the real communicator ---------------------------------------------------------------------------
@pytest.mark.parametrize("k", [31, 63])
def test_world_1_in_batches_equals_preprocess_and_the_oracle(monkeypatch, k):
    small_batches(monkeypatch)
    from sparrowhawk_amd.dist import LibComm
    fq = dataset()
    need = -(-packed_bases(fq, k) // BATCH)
    assert need >= 5
    o = run_oracle([fq], k=k, min_count=3, min_qual=20)
    inputs = inputs_of(fq)
    comm = LibComm(0, 1)
    try:
        for name, (files, markers) in inputs.items():
            want = reference(files, k)
            for split in (1, 0):
                h = sharded(comm, files, k, split=bool(split))
                h.assemble()
                t = h.timings()
                print(name, "split", split, {x: v for x, v in t.items() if x.startswith("shard_fastq")})
                assert (h.get_preprocessing_info(), h.get_assembly()) == want, (name, split)
                assert t["shard_fastq_batches_x1"] >= need, (name, t)
                assert t["shard_fastq_windows_x1"] >= need, (name, t)
                for m, v in markers.items():
                    assert t.get(m, 0) == v, (name, m, t)
                if name == "gz":
                    assert t.get("shard_fastq_member_whole_x1", 0) + t.get("shard_fastq_host_x1", 0) == 1, t
                # SPEC S12: one loop:<reads>:<pct> per batch, reads and pct never fall, the last one says 100, then loop:end
                loops = [s.split(":")[3:] for s in h.states if s.startswith("preprocess:bulk:loop:") and s.split(":")[3].isdigit()]
                assert len(loops) >= need and loops[-1][1] == "100", loops
                assert all(int(x[0]) <= int(y[0]) and int(x[1]) <= int(y[1]) for x, y in zip(loops, loops[1:])), loops
                assert h.states[h.states.index("preprocess:bulk:loop:" + ":".join(loops[-1])) + 1] == "preprocess:bulk:loop:end"
                if split and name == "bgzf":                  # (every input holds the same reads: one comparison with the oracle)
                    compare_all(h, o, check_graph=False)
                h.free()
            assert want == reference(inputs["text"][0], k), name
    finally:
        comm.free()


def test_world_1_in_batches_k127(monkeypatch):
    small_batches(monkeypatch)
    from sparrowhawk_amd.dist import LibComm
    k = 127
    fq = dataset()
    files = (bgzf_write(fq, 4096), None)
    comm = LibComm(0, 1)
    try:
        h = sharded(comm, files, k)
        h.assemble()
        assert (h.get_preprocessing_info(), h.get_assembly()) == reference(files, k)
        assert h.timings()["shard_fastq_batches_x1"] >= -(-packed_bases(fq, k) // BATCH) >= 2
        compare_all(h, run_oracle([fq], k=k, min_count=3, min_qual=20), check_graph=False)
        h.free()
    finally:
        comm.free()


def test_the_same_inputs_take_one_batch_where_they_fit(monkeypatch):
    monkeypatch.delenv("SHK_BATCH_BASES", raising=False)
    monkeypatch.setenv("SHK_GUNZIP_DEVICE_MIN", "4096")
    from sparrowhawk_amd.dist import LibComm
    fq = dataset()
    comm = LibComm(0, 1)
    try:
        for name, (files, markers) in inputs_of(fq).items():
            h = sharded(comm, files, 31)
            t = h.timings()
            assert t["shard_fastq_batches_x1"] == 1 and t["shard_fastq_windows_x1"] == 1, (name, t)
            for m, v in markers.items():
                assert t.get(m, 0) == v, (name, m, t)
            assert h.get_preprocessing_info() == reference(files, 31)[0], name
            h.free()
    finally:
        comm.free()


# ---- 2. the three record paths, 3. merged batches --------------------------------------------------------------------
@pytest.mark.parametrize("dedupe", ["1", "0"])
@pytest.mark.parametrize("merge_at", [None, "3"])
def test_deduplicated_and_raw_records_from_several_batches(monkeypatch, dedupe, merge_at):
    """SHK_SHARD_DEDUPE = 1: the view over the batches' dense buffers is deduplicated; = 0: the raw records are copied from
    them into the send buffer.  SHK_MERGE_BATCHES_AT = 3 with seven batches and more: the batches are merged on the way."""
    small_batches(monkeypatch, 80000 if merge_at else BATCH)
    monkeypatch.setenv("SHK_SHARD_DEDUPE", dedupe)
    if merge_at:
        monkeypatch.setenv("SHK_MERGE_BATCHES_AT", merge_at)
    from sparrowhawk_amd.dist import LibComm
    fq = dataset()
    comm = LibComm(0, 1)
    try:
        for files in ((fq, None), (bgzf_write(fq, 4096), None)):
            h = sharded(comm, files, 31)
            h.assemble()
            t = h.timings()
            assert t["shard_fastq_batches_x1"] >= (7 if merge_at else 6), t
            assert t["shard_records_deduplicated_x1"] == float(dedupe), t
            assert ("batch_merge_kernel" in t) == bool(merge_at), t
            assert (h.get_preprocessing_info(), h.get_assembly()) == reference(files, 31)
            h.free()
    finally:
        comm.free()


def test_bloom_mode_from_several_batches(monkeypatch):
    """Bloom mode sends raw records.  SPEC S4 as test_bloom_mode_* checks it where the rows stay sharded: the instance total is
    exact, no count is lost (the histogram's mass only ever moves up), nkmers is at least the exact value."""
    small_batches(monkeypatch)
    from sparrowhawk_amd.dist import LibComm
    fq = dataset()
    mc = 3
    o = run_oracle([fq], k=31, min_count=mc, min_qual=20)
    comm = LibComm(0, 1)
    try:
        h = sharded(comm, (bgzf_write(fq, 4096), None), 31, do_bloom=True, min_count=mc)
        t = h.timings()
        assert h.states[1] == "preprocess:bloom:start"
        assert t["shard_fastq_batches_x1"] >= 6 and t["shard_records_deduplicated_x1"] == 0.0, t
        assert h.total_instances == o.total_instances
        hist, ohist = h.histo().astype(np.int64), o.histo().astype(np.int64)
        w = np.arange(1, 501)
        assert int((hist * w).sum()) >= int((ohist * w).sum())                  # counts are exact or one too high, never too low
        assert int(hist[mc:].sum()) >= int(ohist[mc:].sum())                    # no k-mer above the threshold is lost
        assert int(hist[1:].sum()) <= int(ohist[1:].sum()) + int(ohist[0])      # only singletons can have moved up
        nk, onk = json.loads(h.get_preprocessing_info()), json.loads(o.preprocessing_json())
        key = [x for x in onk if "kmers" in x.lower()][0]
        assert nk[key] >= onk[key], (nk, onk)
        h.free()
    finally:
        comm.free()


# ---- 4. shk_shard_preprocess_batches ---------------------------------------------------------------------------------
def test_packed_reads_in_three_batches_equal_one(monkeypatch):
    import torch
    from sparrowhawk_amd.dist import LibComm, sharded_preprocess_batches, sharded_preprocess_rccl
    k = 31
    fq = dataset()
    dev = torch.device("cuda", 0)
    c1 = fq.find(b"\n@r", len(fq) // 5) + 1
    c2 = fq.find(b"\n@r", len(fq) * 2 // 3) + 1
    comm = LibComm(0, 1)
    try:
        def up(text):
            bases, seg, nb, nr = pack_fastq(text, k, 20)
            return (torch.from_numpy(bases.view(np.int32)).to(dev), torch.from_numpy(seg.view(np.int32)).to(dev), len(seg) - 1, nb, nr)
        whole = up(fq)
        parts = [up(fq[:c1]), up(fq[c1:c2]), up(fq[c2:])]
        torch.cuda.synchronize()
        assert sum(p[4] for p in parts) == whole[4] and sum(p[3] for p in parts) == whole[3]
        h = AssemblyHelper.new(k, True, 3, 20, 0, False, False, False, False)
        sharded_preprocess_rccl(h, whole[0].data_ptr(), whole[1].data_ptr(), whole[2], whole[3], whole[4], comm)
        h.assemble()
        want = (h.get_preprocessing_info(), h.get_assembly(), h.total_instances)
        one_states = h.states
        h.free()
        for dedupe in ("1", "0"):
            monkeypatch.setenv("SHK_SHARD_DEDUPE", dedupe)
            h = AssemblyHelper.new(k, True, 3, 20, 0, False, False, False, False)
            sharded_preprocess_batches(h, comm, [(p[0].data_ptr(), p[1].data_ptr(), p[2], p[3]) for p in parts], whole[4])
            h.assemble()
            assert (h.get_preprocessing_info(), h.get_assembly(), h.total_instances) == want, dedupe
            loops = [s for s in h.states if s.startswith("preprocess:bulk:loop:") and s.split(":")[3].isdigit()]
            assert len(loops) == 3 and loops[-1] == "preprocess:bulk:loop:%d:100" % whole[4], loops
            assert [s for s in h.states if s not in loops] == [s for s in one_states if s != loops[-1]]
            h.free()
        monkeypatch.delenv("SHK_SHARD_DEDUPE")
        # no batch at all: the empty result that n_seg == 0 gives
        h0 = AssemblyHelper.new(k, True, 3, 20, 0, False, False, False, False)
        sharded_preprocess_rccl(h0, None, None, 0, 0, 0, comm)
        h0.assemble()
        h1 = AssemblyHelper.new(k, True, 3, 20, 0, False, False, False, False)
        sharded_preprocess_batches(h1, comm, [], 0)
        h1.assemble()
        assert (h1.get_preprocessing_info(), h1.get_assembly(), h1.states) == (h0.get_preprocessing_info(), h0.get_assembly(), h0.states)
        # a batch of 2^32 bases or more is refused with the message of the one-batch call
        h2 = AssemblyHelper.new(k, False, 3, 20, 0, False, False, False, False)
        with pytest.raises(ShkError) as ei:
            sharded_preprocess_batches(h2, comm, [(parts[0][0].data_ptr(), parts[0][1].data_ptr(), parts[0][2], parts[0][3]),
                                                  (parts[1][0].data_ptr(), parts[1][1].data_ptr(), parts[1][2], 1 << 32)], whole[4])
        assert ei.value.code == -1 and "batch too large" in str(ei.value), ei.value
        for x in (h0, h1, h2):
            x.free()
    finally:
        comm.free()


# ---- 5. edges of the cutting -----------------------------------------------------------------------------------------
def records(fq):
    lines = fq.split(b"\n")
    assert lines[-1] == b"" and (len(lines) - 1) % 4 == 0
    return [b"\n".join(lines[i:i + 4]) + b"\n" for i in range(0, len(lines) - 1, 4)]


def dead_records(n, what):
    """reads without a valid base: all N, or every quality below min_qual"""
    if what == "N":
        return [b"@n%d\n" % i + b"N" * 150 + b"\n+\n" + b"I" * 150 + b"\n" for i in range(n)]
    return [b"@q%d\n" % i + b"ACGT" * 37 + b"AC\n+\n" + b"#" * 150 + b"\n" for i in range(n)]


def edge_cases(lib):
    recs = records(dataset())
    n = len(recs)
    piece = 2 * BATCH                                        # bytes of text per piece and per window
    cases = {}
    for what in ("N", "lowq"):
        dead = dead_records(1500, what)                      # ~ 470 kB: two whole pieces and more
        assert sum(map(len, dead)) > 2 * piece
        cases["a stretch without a valid base (%s)" % what] = b"".join(recs[:n // 2] + dead + recs[n // 2:])
    rng = np.random.default_rng(5)
    short = [b"@s%d\n" % i + bytes(rng.choice(list(b"ACGT"), ln).tolist()) + b"\n+\n" + b"I" * ln + b"\n" for i, ln in enumerate(rng.integers(1, 31, 900))]
    mixed = [r for pair in zip(recs, short + [b""] * (n - len(short))) for r in pair]
    cases["reads shorter than k"] = b"".join(mixed)
    cases["a last record without a line end"] = b"".join(recs)[:-1]
    # the last piece holds a single record: the pieces are cut as the library cuts plain text (the last record start inside
    # `piece` bytes), and the text ends with the record in which a piece's view ends — where that record is the one the cut
    # falls on (tried with short reads of a few lengths in front of that piece)
    def cut_points(t):
        cuts, frm = [0], 0
        while len(t) - frm > piece:
            at = int(lib.shk_host_last_record_start(t[frm:frm + piece], piece))
            assert 0 < at < piece
            frm += at
            cuts.append(frm)
        return cuts
    single = None
    whole = b"".join(recs)
    at2 = cut_points(whole)[2]
    for fill in range(10, 400, 40):                          # (a short read in front of the third piece moves its cut against its records)
        t = whole[:at2] + b"@fill\n" + b"A" * fill + b"\n+\n" + b"I" * fill + b"\n" + whole[at2:]
        cuts = cut_points(t)
        cand = t[:t.find(b"\n@r", cuts[2] + piece) + 1]
        if cand[cut_points(cand)[-1]:].count(b"\n") == 4:
            single = cand
            break
    assert single is not None
    cases["a last piece of a single record"] = single
    cases["CRLF line ends"] = b"".join(recs[:n * 2 // 3]).replace(b"\n", b"\r\n")
    return cases


def test_edges_of_the_cutting(lib, monkeypatch):
    small_batches(monkeypatch)
    from sparrowhawk_amd.dist import LibComm
    k = 31
    comm = LibComm(0, 1)
    try:
        for name, text in edge_cases(lib).items():
            forms = {"text": (text, None), "bgzf": (bgzf_write(text, 4096), None)}
            if name.startswith("a stretch"):
                forms["gz"] = (gzip.compress(text, compresslevel=6), None)
            for form, files in forms.items():
                h = sharded(comm, files, k)
                h.assemble()
                t = h.timings()
                print(name, form, {x: v for x, v in t.items() if x.startswith("shard_fastq")})
                assert t["shard_fastq_batches_x1"] >= 3, (name, form, t)
                assert (h.get_preprocessing_info(), h.get_assembly()) == reference(files, k), (name, form)
                h.free()
        # a pair whose first file ends without a newline: the files go one after the other
        a, b = halves(dataset())
        for files in ((a[:-1], b), (bgzf_write(a[:-1], 4096), bgzf_write(b, 3000, level=1))):
            h = sharded(comm, files, k)
            h.assemble()
            assert h.timings()["shard_fastq_batches_x1"] >= 6
            assert (h.get_preprocessing_info(), h.get_assembly()) == reference(files, k)
            h.free()
    finally:
        comm.free()


def test_text_that_turns_irregular_in_a_later_window_goes_to_the_host_parser(monkeypatch):
    small_batches(monkeypatch)
    from sparrowhawk_amd.dist import LibComm
    recs = records(dataset())
    n = len(recs)
    text = b"".join(recs[:n // 2]) + b"\n".join(recs[n // 2:])      # blank lines between the records from the middle on
    comm = LibComm(0, 1)
    try:
        for files in ((text, None), (bgzf_write(text, 4096), None), (gzip.compress(text), None)):
            h = sharded(comm, files, 31)
            h.assemble()
            t = h.timings()
            assert t.get("shard_fastq_host_x1", 0) == 1 and t["shard_fastq_batches_x1"] >= 6, t
            assert t["shard_fastq_windows_x1"] >= 2, t                           # the first windows went through the device parser
            assert (h.get_preprocessing_info(), h.get_assembly()) == reference(files, 31)
            h.free()
    finally:
        comm.free()


# ---- 6. worlds of 2 and 3 over the stand-in transport ----------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
def test_several_ranks_with_several_batches_each(monkeypatch, world):
    """(A) split = 1, the same BGZF pair on every rank, every rank in several batches.  (B) split = 0: rank 0 a file of several
    batches, rank 1 none, rank 2 (world 3) a file that fits one batch.  (C) rank 1's file ends inside a record near its END:
    its first windows parse, the failure travels with the size exchange.  (D) SHK_FAULT_INJECT=pass1 on rank 0."""
    from test_dist import mock_rccl_library
    k = 31
    fq = dataset(seed=40 + world)
    a, b = halves(fq)
    small_cut = fq.find(b"\n@r", len(fq) * 9 // 10) + 1
    big, small = fq[:small_cut], fq[small_cut:]
    assert packed_bases(small, k) < BATCH < packed_bases(a, k) // 2
    cut = a[:a.rfind(b"\n@r") + 1 + 40]                      # ends inside a sequence line
    with pytest.raises(ShkError) as ei:
        pack_fastq(cut, k, 20)
    parser_message = str(ei.value)
    assert "SHK_E_PARSE" in parser_message
    small_batches(monkeypatch)
    monkeypatch.setenv("SHK_RCCL_LIBRARY", mock_rccl_library())
    with tempfile.TemporaryDirectory() as d:
        def put(name, data):
            p = os.path.join(d, name)
            open(p, "wb").write(data)
            return p
        za, zb = bgzf_write(a, 4096), bgzf_write(b, 4096)
        pa, pb = put("a.fq.gz", za), put("b.fq.gz", zb)
        ta, tb, tcut = put("a.fq", a), put("b.fq", b), put("cut.fq", cut)
        own = [[put("big.fq.gz", bgzf_write(big, 4096)), None], None, [put("small.fq", small), None]] if world == 3 else [[put("ab.fq.gz", bgzf_write(fq, 4096)), None], None]
        bad = [[ta, None], [tcut, None], [tb, None]][:world]
        cases = [{"files": [[pa, pb]] * world, "split": 1},
                 {"files": own, "split": 0},
                 {"files": bad, "split": 0},
                 {"files": [[pa, pb]] * world, "split": 1, "inject": {"rank": 0, "step": "pass1"}}]
        for cs in cases:
            cs.update(k=k, min_count=3)
        cfgp = put("cfg.json", json.dumps({"cases": cases}).encode())
        out = os.path.join(d, "res")
        launch(world, [out, cfgp], 29940 + world, timeout=240)
        res = [json.load(open(f"{out}.{r}")) for r in range(world)]
    o = run_oracle([fq], k=k, min_count=3, min_qual=20)
    o.assemble()
    size = len(za) + len(zb)
    for r in range(world):
        for case in (0, 1):
            x = res[r][case]
            assert "error" not in x, (r, case, x)
            assert x["pre"] == o.preprocessing_json() and x["asm"] == o.assembly_json(), (r, case)
        t = res[r][0]["timings"]
        assert t.get("shard_fastq_bgzf_slice_x1", 0) == 2 and t["shard_fastq_batches_x1"] >= 2, t
        if world == 3:
            assert t["shard_fastq_uploaded_bytes"] <= 0.6 * size, (t, size)      # a rank uploads its runs and a few blocks, not the files
        t = res[r][1]["timings"]
        assert t["shard_fastq_batches_x1"] >= (5 if r == 0 else 1), (r, t)
        x = res[r][2]
        assert "error" in x, (r, x)
        if r == 1:
            assert x["code"] == -3 and x["error"] == parser_message, x
        else:
            assert "another rank failed" in x["error"], x
        x = res[r][3]
        assert "error" in x, (r, x)
        assert ("injected fault" if r == 0 else "another rank failed during pass 1") in x["error"], x
