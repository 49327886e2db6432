"""The sharded assembly with the chains of its unitig graph walked and laid out on the device (the flat form of
UnitigGraphResult, csrc/unitig_graph_gpu.hip): a one-rank communicator, the oracle's bytes, and the timing entries that say
which walk ran.  The cases are those of test_gpu_shard_unitig_device.py (computed once for both files)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_shard_unitig_device import _assemble_sharded, _cases

pytestmark = pytest.mark.gpu


def test_sharded_assembly_with_the_chains_walked_on_the_device(monkeypatch):
    from sparrowhawk_amd.dist import LibComm
    monkeypatch.setenv("SHK_UNITIG_DEVICE", "1")
    monkeypatch.delenv("SHK_UNITIG_CHAINS_DEVICE", raising=False)
    comm = LibComm(0, 1)
    try:
        cases = _cases()
        assert len(cases) == 42
        for i, (fq, pr, (pre, asm)) in enumerate(cases):
            got_pre, got_asm, timings = _assemble_sharded(comm, fq, pr)
            assert got_pre == pre, (i, pr)
            assert got_asm == asm, (i, pr)
            assert timings.get("shard_graph_unitig_chains_device_x1") == 1, (i, timings)
            assert timings.get("shard_graph_unitig_device_x1") == 1, (i, timings)
            assert timings["shard_graph_unitig_contigs_x1"] >= 0
    finally:
        comm.free()


def test_sharded_assembly_with_the_chains_walked_on_the_host(monkeypatch):
    from sparrowhawk_amd.dist import LibComm
    monkeypatch.setenv("SHK_UNITIG_DEVICE", "1")
    monkeypatch.setenv("SHK_UNITIG_CHAINS_DEVICE", "0")
    comm = LibComm(0, 1)
    try:
        cases = _cases()
        for i in (0, 13, 27, 40, 41):                         # three random graphs and the two chromosomes
            fq, pr, (pre, asm) = cases[i]
            got_pre, got_asm, timings = _assemble_sharded(comm, fq, pr)
            assert got_pre == pre and got_asm == asm, (i, pr)
            assert "shard_graph_unitig_chains_device_x1" not in timings, (i, timings)
            assert timings.get("shard_graph_unitig_device_x1") == 1, (i, timings)
            assert "shard_graph_unitig_contigs_x1" in timings
    finally:
        comm.free()
