"""The sharded assembly with get_assembly() written on the device from the all-reduced contig text (csrc/writer_text_gpu.h;
SHK_DEVICE_WRITER_MIN, SHK_SHARD_DEVICE_WRITER): a one-rank communicator, the oracle's bytes, and the timing entries that
say which writer ran.  The stage is local and works on text that is identical on every rank, so one rank shows all of it."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_gpu_shard_unitig_device import _assemble_sharded, _cases      # (the 40 small graphs and the two chromosomes, with the oracle's texts)

pytestmark = pytest.mark.gpu


def _run_family(indices, expect_device):
    from sparrowhawk_amd.dist import LibComm
    comm = LibComm(0, 1)
    n_written = 0
    try:
        cases = _cases()
        for i in (range(len(cases)) if indices is None else indices):
            fq, pr, (pre, asm) = cases[i]
            got_pre, got_asm, timings = _assemble_sharded(comm, fq, pr)
            assert got_pre == pre, (i, pr)
            assert got_asm == asm, (i, pr)
            assert "shard_writer_device_declined_x1" not in timings, (i, timings)
            if expect_device and '"ncontigs":0,' not in asm:           # (no contig: there is no text to write from)
                assert timings.get("shard_writer_device_x1") == 1, (i, timings)
                assert timings["outputs_host_clock"] == 0, (i, timings)
                for name in ("device_writer_d2h_host_clock", "device_writer_json_MB", "device_writer_links_x1e-3"):
                    assert name in timings, (i, name, timings)         # (device_writer_kernels comes with the stage timers of a verbose handle)
                n_written += 1
            else:
                assert "shard_writer_device_x1" not in timings, (i, timings)
    finally:
        comm.free()
    return n_written


@pytest.mark.parametrize("unitig_device,chains_device", [(None, None), ("1", None), ("1", "0")])
def test_sharded_assembly_written_on_the_device(monkeypatch, unitig_device, chains_device):
    """forced on for every assembly that has a contig; with the unitig graph on the host (per-contig records feed the
    writer), on the device (the flat form does), and on the device with the chains walked by the host"""
    monkeypatch.setenv("SHK_DEVICE_WRITER_MIN", "1")
    monkeypatch.delenv("SHK_SHARD_DEVICE_WRITER", raising=False)
    for name, v in (("SHK_UNITIG_DEVICE", unitig_device), ("SHK_UNITIG_CHAINS_DEVICE", chains_device)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, v)
    assert _run_family(None, True) >= 30


@pytest.mark.parametrize("forced_off", [True, False])
def test_sharded_assembly_written_on_the_host(monkeypatch, forced_off):
    """switched off although the threshold is met, and with both variables unset (these assemblies lie far below 20 000
    contigs): the text is downloaded and the host writer runs, as before"""
    if forced_off:
        monkeypatch.setenv("SHK_DEVICE_WRITER_MIN", "1")
        monkeypatch.setenv("SHK_SHARD_DEVICE_WRITER", "0")
    else:
        monkeypatch.delenv("SHK_DEVICE_WRITER_MIN", raising=False)
        monkeypatch.delenv("SHK_SHARD_DEVICE_WRITER", raising=False)
    monkeypatch.delenv("SHK_UNITIG_DEVICE", raising=False)
    _run_family((0, 13, 27, 40, 41), False)


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_assembly_written_on_the_device_on_every_rank(monkeypatch, world):
    """several ranks (on the one GPU, bytes through tests/mock_rccl, the worker of test_dist.py as it is): the circular
    chromosome with two plasmids — every rank writes the text from its own copy of the all-reduced contigs, returns the
    oracle's bytes and reports the marker"""
    import json
    import tempfile
    from test_dist import _write_cases, launch, mock_rccl_library
    fq, pr, (pre, asm) = _cases()[40]
    monkeypatch.setenv("SHK_DEVICE_WRITER_MIN", "1")
    monkeypatch.delenv("SHK_SHARD_DEVICE_WRITER", raising=False)
    monkeypatch.setenv("SHK_RCCL_LIBRARY", mock_rccl_library())
    with tempfile.TemporaryDirectory() as d:
        cfgp = _write_cases(d, [(fq, dict(pr, timings=True))])
        out = os.path.join(d, "res")
        launch(world, ["rccl_many", out, cfgp], 29830 + world, timeout=300)
        res = [json.load(open(f"{out}.{r}"))[0] for r in range(world)]
    for r in range(world):
        assert "error" not in res[r], (r, res[r])
        assert res[r]["pre"] == pre and res[r]["asm"] == asm, r
        assert res[r]["timings"].get("shard_writer_device_x1") == 1, (r, res[r]["timings"])
        assert "shard_writer_device_declined_x1" not in res[r]["timings"]
        assert res[r]["timings"]["outputs_host_clock"] == 0


def test_sharded_assembly_without_a_solid_kmer(monkeypatch):
    """no contig at all: the JSON of an empty assembly, from the host writer, whatever the threshold says"""
    from sparrowhawk_amd import synth
    from sparrowhawk_amd.dist import LibComm
    from test_dist import _oracle_jsons
    monkeypatch.setenv("SHK_DEVICE_WRITER_MIN", "1")
    g = synth.random_genome(3000, 4)
    codes, quals = synth.sample_reads(g, 10, 100, 5, err=0.0)           # (coverage far below min_count: nothing is solid)
    fq = synth.to_fastq(codes, quals)
    pr = dict(k=31, min_count=50, min_qual=20)
    pre, asm = _oracle_jsons(fq, pr)
    assert '"ncontigs":0,' in asm
    comm = LibComm(0, 1)
    try:
        got_pre, got_asm, timings = _assemble_sharded(comm, fq, pr)
    finally:
        comm.free()
    assert got_pre == pre and got_asm == asm
    assert "shard_writer_device_x1" not in timings and "shard_writer_device_declined_x1" not in timings
