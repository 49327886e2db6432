"""The graph partitions taken from the counting pass (build_graph, graph_part.h): when every counting group left
k_count_weighted in one piece, its row range is a graph partition and the regrouping kernels do not run
(timings: graph_partitions_from_counting_x1); otherwise the graph partitions are cut as before
(graph_partitions_cut_x1).  Either way the graph, the corrected graph and the assembly are the oracle's."""
import json
import os

import numpy as np
import pytest

from sparrowhawk_amd import AssemblyHelper
from util import compare_all, make_dataset, run_oracle, sorted_table

pytestmark = pytest.mark.gpu

RANGES = "graph_partitions_from_counting_x1"
REGROUPED = "graph_partitions_cut_x1"


def product(fq, k, min_count, env=None, min_qual=20):
    old = {key: os.environ.get(key) for key in (env or {})}
    os.environ.update({key: str(v) for key, v in (env or {}).items()})
    try:
        h = AssemblyHelper.new(k, True, min_count, min_qual, 0, False, False, False, False)
        h.preprocess(fq, None)
        h.assemble()
        return h
    finally:
        for key, v in old.items():
            if v is None:
                os.environ.pop(key, None)
            else:
                os.environ[key] = v


def path_of(h):
    t = h.timings()
    return t.get(RANGES, 0), t.get(REGROUPED, 0)


@pytest.mark.parametrize("k", [31, 51])
def test_ranges_path_matches_oracle_and_old_path(k):
    """A clean isolate: the counting groups become the graph partitions, and the result equals the oracle's and that
    of the partitions cut by k_gp_count (SHK_GRAPH_RANGES=0), adjacency byte by byte."""
    g, fq = make_dataset(60000, 40, err=0.0, seed=300 + k)
    h = product(fq, k, 3)
    assert path_of(h) == (1, 0), h.timings()
    o = run_oracle([fq], k=k, min_count=3)
    compare_all(h, o)
    old = product(fq, k, 3, {"SHK_GRAPH_RANGES": 0})
    assert path_of(old) == (0, 1), old.timings()
    assert old.get_assembly() == h.get_assembly()
    # (row order: the order in which the counting groups were emitted, which varies from run to run — compared in key order)
    _, _, o_new = sorted_table(*h.solid())
    _, _, o_old = sorted_table(*old.solid())
    for x, y in zip(h.adjacency(), old.adjacency()):
        assert np.array_equal(x[o_new], y[o_old])


@pytest.mark.parametrize("k", [31, 51])
def test_ranges_path_partitions_beyond_the_lds_table(k):
    """Partitions whose mini table does not fit the LDS one (here: cut down to 64 slots) build it in global memory and
    send all their neighbour candidates to k_graph_remote; the result does not change."""
    g, fq = make_dataset(40000, 40, err=0.003, seed=400 + k)
    h = product(fq, k, 3, {"SHK_GRAPH_LDS_SLOTS": 64})
    assert path_of(h) == (1, 0), h.timings()
    assert h.n_solid > 64 * 64 // 2                         # more rows than 64 partitions of <= 32 rows hold
    o = run_oracle([fq], k=k, min_count=3)
    compare_all(h, o)


def test_error_rich_reads_fall_back():
    """Counting partitions that overflow the LDS table go to the k-mer-level repartition: their rows are not where the
    ranges say, so the graph partitions are cut from the rows as before — with the oracle's result."""
    g, fq = make_dataset(60000, 20, err=0.02, seed=501)
    h = product(fq, 31, 2, {"SHK_PART_P": 16}, min_qual=0)          # (min_qual 0: the errors are not masked)
    t = h.timings()
    assert t.get("count_repartitioned_x1", 0) > 0, t
    assert path_of(h) == (0, 1), t
    o = run_oracle([fq], k=31, min_count=2, min_qual=0)
    compare_all(h, o)


def test_forced_partition_sizes_take_the_old_path():
    """SHK_GP_ROWS asks for the graph partitions of k_gp_count, whatever the counting pass left."""
    g, fq = make_dataset(30000, 30, seed=601)
    h = product(fq, 31, 3, {"SHK_GP_ROWS": 64})
    assert path_of(h) == (0, 1), h.timings()
    ref = product(fq, 31, 3)
    assert path_of(ref) == (1, 0)
    assert json.loads(h.get_assembly()) == json.loads(ref.get_assembly())


def test_groups_too_large_for_the_lds_tables_take_the_old_path():
    """Pass 1 sizes the counting groups by instances: few groups of many rows (here 64 of ~2300) would leave nearly
    every mini table in global memory, so the partitions are cut from the rows as before.  Forced onto the groups
    anyway (SHK_GRAPH_RANGE_ROWS), the tables beyond the LDS give the same assembly."""
    g, fq = make_dataset(150000, 20, seed=701)
    h = product(fq, 31, 3, {"SHK_PART_P": 64})
    assert h.n_solid > 64 * 1536
    assert path_of(h) == (0, 1), h.timings()
    forced = product(fq, 31, 3, {"SHK_PART_P": 64, "SHK_GRAPH_RANGE_ROWS": 100000})
    assert path_of(forced) == (1, 0), forced.timings()
    assert forced.get_assembly() == h.get_assembly()
    assert forced.get_preprocessing_info() == h.get_preprocessing_info()


def test_two_partitions_per_counting_table():
    """SHK_COUNT_MERGE=2: a group is two counting partitions whose numbers share their low bits, counted in one table and
    emitted as one range — the graph partition is the group."""
    g, fq = make_dataset(40000, 30, seed=801)
    h = product(fq, 31, 3, {"SHK_COUNT_MERGE": 2, "SHK_PART_P": 4096})
    assert path_of(h) == (1, 0), h.timings()
    o = run_oracle([fq], k=31, min_count=3)
    compare_all(h, o)


def test_sharded_assembly_takes_the_old_path():
    """The sharded assembly cuts its graph partitions from the global node count (every rank the same), never from the
    counting groups; with one rank it gives the bytes of the local path, which takes the groups."""
    import torch
    from sparrowhawk_amd import pack_fastq
    from sparrowhawk_amd.dist import LibComm, sharded_preprocess_rccl
    g, fq = make_dataset(40000, 30, seed=901)
    local = product(fq, 31, 3, min_qual=0)
    assert path_of(local) == (1, 0), local.timings()
    dev = torch.device("cuda", 0)
    comm = LibComm(0, 1)
    try:
        bases, seg, nb, nr = pack_fastq(fq, 31, 0)
        d_bases = torch.from_numpy(bases.view(np.int32)).to(dev)
        d_seg = torch.from_numpy(seg.view(np.int32)).to(dev)
        torch.cuda.synchronize()
        h = AssemblyHelper.new(31, False, 3, 0, 0, False, False, False, False)
        sharded_preprocess_rccl(h, d_bases.data_ptr(), d_seg.data_ptr(), len(seg) - 1, nb, nr, comm)
        h.assemble()
        assert "shard_graph_stitch" in h.timings()
        assert path_of(h) == (0, 1), h.timings()
        assert h.get_assembly() == local.get_assembly()
        h.free()
    finally:
        comm.free()
