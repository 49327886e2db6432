"""The sharded assembly with its unitig graph corrected on the device (SHK_UNITIG_DEVICE, csrc/unitig_graph_gpu.hip): a
one-rank communicator, the oracle's bytes, and the timing entries that say which path ran.  The stage is local and works
on records that are identical on every rank, so one rank shows all of it; the exchange code around it keeps its own tests
(test_dist.py), on the host path."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_dist import _graph_cases, _oracle_jsons

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _cases():
    """40 random small graphs, and the circular chromosome with two plasmids of test_sharded_graph_several_ranks — clean, and
    with errors at k = 51 — each with the oracle's two texts (computed once for both tests)"""
    from sparrowhawk_amd import synth
    cases = _graph_cases(8300, 40)
    for seed, err, k, mc in ((31, 0.0, 31, 3), (33, 0.005, 51, 2)):
        chrom = synth.random_genome(60000, seed)
        p1, p2 = synth.random_genome(5000, seed + 100), synth.random_genome(700, seed + 200)
        recs = []
        for j, (g, cov) in enumerate(((chrom, 40), (p1, 60), (p2, 80))):
            codes, quals = synth.sample_reads(g, len(g) * cov // 150, 150, seed * 10 + j, err=err, circular=True)
            recs.extend(synth.to_fastq(codes, quals).decode().split("@r")[1:])
        cases.append((("@r" + "@r".join(recs)).encode(), dict(k=k, min_count=mc, min_qual=20)))
    return tuple((fq, pr, _oracle_jsons(fq, pr)) for fq, pr in cases)


def _assemble_sharded(comm, fq, pr):
    import torch
    from sparrowhawk_amd import AssemblyHelper, pack_fastq
    from sparrowhawk_amd.dist import sharded_preprocess_rccl
    dev = torch.device("cuda", 0)
    bases, seg, nb, nr = pack_fastq(fq, pr["k"], pr["min_qual"])
    d_bases = torch.from_numpy(bases.view(np.int32)).to(dev)
    d_seg = torch.from_numpy(seg.view(np.int32)).to(dev)
    torch.cuda.synchronize()
    h = AssemblyHelper.new(pr["k"], False, pr["min_count"], pr["min_qual"], 0, False, False, pr.get("no_bubble_collapse", False),
                           pr.get("no_dead_end_removal", False))
    try:
        sharded_preprocess_rccl(h, d_bases.data_ptr(), d_seg.data_ptr(), len(seg) - 1, nb, nr, comm)
        h.assemble()
        return h.get_preprocessing_info(), h.get_assembly(), h.timings()
    finally:
        h.free()


def test_sharded_assembly_with_the_unitig_graph_on_the_device(monkeypatch):
    from sparrowhawk_amd.dist import LibComm
    monkeypatch.setenv("SHK_UNITIG_DEVICE", "1")
    comm = LibComm(0, 1)
    try:
        for i, (fq, pr, (pre, asm)) in enumerate(_cases()):
            got_pre, got_asm, timings = _assemble_sharded(comm, fq, pr)
            assert got_pre == pre, (i, pr)
            assert got_asm == asm, (i, pr)
            assert timings.get("shard_graph_unitig_device_x1") == 1, (i, timings)
            assert "shard_graph_unitig_device_declined_x1" not in timings
            assert timings["shard_graph_unitig_graph"] >= 0
    finally:
        comm.free()


def test_sharded_assembly_keeps_small_graphs_on_the_host_by_default(monkeypatch):
    from sparrowhawk_amd.dist import LibComm
    monkeypatch.delenv("SHK_UNITIG_DEVICE", raising=False)
    monkeypatch.delenv("SHK_UNITIG_DEVICE_MIN", raising=False)
    comm = LibComm(0, 1)
    try:
        cases = _cases()
        for i in (0, 13, 27, 40, 41):                         # three random graphs and the two chromosomes
            fq, pr, (pre, asm) = cases[i]
            got_pre, got_asm, timings = _assemble_sharded(comm, fq, pr)
            assert got_pre == pre and got_asm == asm, (i, pr)
            assert "shard_graph_unitig_device_x1" not in timings, (i, timings)
            assert "shard_graph_unitig_graph" in timings
    finally:
        comm.free()
