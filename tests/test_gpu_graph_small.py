"""The one-GPU graph stage (csrc/pipeline.hip, graph_part.h, collapse.h, writer_gpu.h) on the adversarial small graphs of
test_oracle._random_graph_case — hairpins, direct and tandem repeats, rings shorter than a read, low coverage, k = 15 ... 41,
both correction switches — through every path of the product that the environment can select, on handles with and without
stage inspection, against the oracle (which tests/pygraph.py pins on this very family).  Bit-exact throughout.
Run on the MI355X box: pytest -m gpu tests/test_gpu_graph_small.py"""
import json

import numpy as np
import pytest

from sparrowhawk_amd import AssemblyHelper, pack_fastq, synth
from test_oracle import SMALL_GRAPH_CASES, small_graph_cases, wide_graph_cases, WIDE_BLOCKS
from util import compare_all, run_oracle, with_env

pytestmark = pytest.mark.gpu

# name -> (environment, run_case keywords).  What each must leave in timings(): MARKERS below.
VARIANTS = [
    ("cut", {"SHK_GRAPH_RANGES": 0}, {}),
    ("tiny_parts", {"SHK_GP_ROWS": 16}, {}),
    ("lds_small", {"SHK_GRAPH_LDS_SLOTS": 64}, {}),                 # tables beyond the LDS one work in global memory
    ("regroup", {"SHK_REGROUP_ROWS": 1}, {}),
    ("no_scan", {"SHK_GRAPH_RANGES": 0, "SHK_REGROUP_ROWS": 0, "SHK_KEEP_SCAN": 0}, {}),
    ("scattered", {"SHK_PART_P": 2}, {}),
    ("tile1_all_split", {"SHK_TILE_ROWS": 1, "SHK_SPLIT_LOG": 0}, {}),
    ("tile3_no_split", {"SHK_TILE_ROWS": 3, "SHK_SPLIT_LOG": 14}, {}),
    ("tile17", {"SHK_TILE_ROWS": 17, "SHK_SPLIT_LOG": 3}, {}),
    ("seg_cap1", {"SHK_SEG_CAP": 1}, {}),
    ("seg_cap8_all_split", {"SHK_SEG_CAP": 8, "SHK_SPLIT_LOG": 0, "SHK_TILE_ROWS": 64}, {}),
    ("plan", {"SHK_DEVICE_PLAN": 1}, {}),
    ("plan_after_retry", {"SHK_DEVICE_PLAN": 1, "SHK_SEG_CAP": 1, "SHK_TILE_ROWS": 3}, {}),
    ("device_writer", {"SHK_DEVICE_WRITER_MIN": 1}, {}),
    ("device_writer_tiles", {"SHK_DEVICE_WRITER_MIN": 1, "SHK_TILE_ROWS": 1, "SHK_SPLIT_LOG": 0}, {}),
    ("arrival", {"SHK_ARRIVAL_MIN": 1}, {}),
    ("arrival_one_block", {"SHK_ARRIVAL_MIN": 1, "SHK_ARRIVAL_BLOCKS": 1, "SHK_WRITER_PAR_MIN": 1}, {}),
    ("shipped", {}, dict(shipped=True, entry="packed_device")),
    ("shipped_plan", {"SHK_DEVICE_PLAN": 1}, dict(shipped=True, entry="packed_host")),
    ("packed_device_verbose", {}, dict(entry="packed_device")),
]
VARIANT = {name: (env, kw) for name, env, kw in VARIANTS}
# every knob a variant or an edge test turns: a run that does not name one runs with it unset (the "empty environment")
KNOBS = sorted({k for _, env, _ in VARIANTS for k in env})


class Facts:
    """What the marker conditions may know about a case: the ORACLE's answer, never the product's."""
    def __init__(self, o):
        ref = json.loads(o.assembly_json())
        self.ncontigs = ref["ncontigs"]
        self.n_solid = len(o.alive())                                # nodes of the graph as built
        self.alive = int(np.count_nonzero(o.alive()))                # nodes left after correction
        links = [l.split("\t") for l in ref["outgfa"].split("\n") if l.startswith("L\t")]
        self.self_links = sum(1 for f in links if f[1] == f[3] and f[2] == f[4])        # rings: a contig linked to itself on one strand


# A chain record exists once per strand of a unitig (collapse.h, k_rank_tails: one per chain; k_orphan_cycles gives a ring
# without a sampled node ONE record, for the strand that is emitted).  So records <= 2 x ncontigs, and records >= ncontigs.
def _retry_seg_cap1(f):
    # SHK_SEG_CAP=1: every contig brings at least one entry of the splitter list (a head per strand of a linear chain, a sampled
    # node or the orphan-ring entry of a ring), two contigs at least two: flag 4 (k_local_frag) or flag 2 (k_orphan_cycles)
    return f.ncontigs >= 2


def _retry_seg_cap8_all_split(f):
    # SHK_SPLIT_LOG=0 makes every alive oriented node a splitter (node_sampled with mask 0), so the list holds exactly
    # 2 x alive nodes and the room of 8 is exceeded (k_local_frag: *n_spl_p > seg_cap) where that is above 8.  Two contigs of
    # one or two nodes each fit: "ncontigs >= 2" alone would be wrong for such a case.
    return 2 * f.alive > 8


def _planned(f):
    # k_plan_emit plans where 1 <= records <= 512 and the text fits n + 512 (k - 1) + 64: certain for 1 <= ncontigs <= 256
    # (no chain record at all — nothing solid, or everything removed — is "not planned": nh == 0)
    return 1 <= f.ncontigs <= 256


def _not_planned(f):
    # ... and declines where records > 512 (nh > max_heads): certain for ncontigs > 512
    return f.ncontigs > 512


def _device_writer(f):
    # pipeline.hip, rank_chains: the chain records stay on the device where n_heads >= 2 x SHK_DEVICE_WRITER_MIN = 2.  Two
    # contigs have two records; ONE contig has two unless it is a ring without a sampled node (one record, k_orphan_cycles) —
    # a linear contig always has its two strands.  So: not asserted for an assembly that is a single circular contig.
    return f.ncontigs >= 2 or (f.ncontigs == 1 and f.self_links == 0)


def _graph_built(f):
    # pipeline.hip, build_graph: the partitions are cut (and the markers set) only where there is a solid k-mer: `if (n || sh_active_)`
    return f.n_solid > 0


def _text_to_send(f):
    # pipeline.hip, collapse: the arrival path lies inside `if (!emitted.empty())`
    return f.ncontigs >= 1


# name -> [(marker, must it be present?, condition on the oracle's facts)]
MARKERS = {
    "cut": [("graph_partitions_cut_x1", True, _graph_built), ("graph_partitions_from_counting_x1", False, _graph_built)],
    "tiny_parts": [("graph_partitions_cut_x1", True, _graph_built)],
    "regroup": [("graph_rows_regrouped_x1", True, _graph_built)],
    "no_scan": [("graph_partitions_cut_x1", True, _graph_built), ("graph_rows_regrouped_x1", False, _graph_built)],
    "seg_cap1": [("collapse_seg_cap_retry_x1", True, _retry_seg_cap1)],
    "seg_cap8_all_split": [("collapse_seg_cap_retry_x1", True, _retry_seg_cap8_all_split)],
    "plan": [("collapse_planned_on_device_x1", True, _planned), ("collapse_planned_on_device_x1", False, _not_planned)],
    "plan_after_retry": [("collapse_planned_on_device_x1", True, _planned), ("collapse_planned_on_device_x1", False, _not_planned),
                         ("collapse_seg_cap_retry_x1", True, _retry_seg_cap1)],
    "device_writer": [("device_writer_kernels", True, _device_writer)],
    "device_writer_tiles": [("device_writer_kernels", True, _device_writer)],
    "arrival": [("collapse_ends_host_clock", True, _text_to_send)],
    "arrival_one_block": [("collapse_ends_host_clock", True, _text_to_send)],
}


def run_case(fq, k, min_count, flags, env, *, verbose=True, entry="text", shipped=False, min_qual=0):
    """One product run: the handle is made, fed through `entry` and assembled with exactly `env` set (every other knob of
    this file unset), and the environment restored.  shipped: the handle bench.py and batch.py make — quiet, and without the
    SHK_KEEP_STAGES / SHK_STAGE_TIMERS that conftest.py sets for every test (both are read per handle): no event between the
    kernels, no initial adjacency kept, timers deferred."""
    e = {name: None for name in KNOBS}
    e.update(env)
    if shipped:
        e.update(SHK_KEEP_STAGES=None, SHK_STAGE_TIMERS=None)
        verbose = False

    def go():
        h = AssemblyHelper.new(k, verbose, min_count, min_qual, 0, False, False, bool(flags.get("no_bubble_collapse")),
                               bool(flags.get("no_dead_end_removal")))
        if entry == "text":
            h.preprocess(fq)
            h.assemble()
        elif entry == "packed_host":
            bases, seg, nbases, nreads = pack_fastq(fq, k, min_qual)
            h.preprocess_packed_host(bases.ctypes.data, seg.ctypes.data, len(seg) - 1, nbases, nreads)
            h.assemble()
        elif entry == "packed_device":
            import torch
            bases, seg, nbases, nreads = pack_fastq(fq, k, min_qual)
            dev = torch.device("cuda", 0)
            d_bases = torch.from_numpy(bases.view(np.int32)).to(dev); d_seg = torch.from_numpy(seg.view(np.int32)).to(dev)
            torch.cuda.synchronize()
            h.preprocess_packed_device(d_bases.data_ptr(), d_seg.data_ptr(), len(seg) - 1, nbases, nreads)
            h.assemble()                                             # (the reads stay where they are until the assembly is done)
            del d_bases, d_seg
        else:
            raise ValueError(entry)
        return h
    return with_env(e, go)


def check_run(fq, k, min_count, flags, facts, oracle_factory, name, env, kw, what, tally=None, min_qual=0):
    """One run against the oracle.  A verbose handle: every stage (compare_all) and the variant's markers; a shipped one: the
    two texts the product returns.  `what` goes into every message: enough to replay the case."""
    msg = f"{what} k={k} min_count={min_count} flags={flags} variant={name} env={env} {kw}"
    h = run_case(fq, k, min_count, flags, env, min_qual=min_qual, **kw)
    try:
        if kw.get("shipped"):
            o = oracle_factory()
            o.assemble()
            assert h.get_preprocessing_info() == o.preprocessing_json(), msg + ": preprocessing info differs"
            assert h.get_assembly() == o.assembly_json(), msg + ": assembly differs"
            return None
        try:
            compare_all(h, oracle_factory(), check_graph=True)
        except AssertionError as e:
            raise AssertionError(f"{msg}: {e}") from e
        t = h.timings()
        for marker, present, cond in MARKERS.get(name, ()):
            if cond(facts):
                assert (marker in t) == present, f"{msg}: {marker} {'missing' if present else 'present'} (ncontigs {facts.ncontigs}, alive {facts.alive})"
                if tally is not None:
                    key = (name, marker, present)
                    tally[key] = tally.get(key, 0) + 1
        return t
    finally:
        h.free()


def _oracle_factory(fq, k, min_count, flags, min_qual=0):
    # (compare_all runs the oracle's assemble itself, on an oracle that has only counted: one per comparison; the oracle takes
    # tens of milliseconds on these inputs)
    return lambda: run_oracle([fq], k=k, min_count=min_count, min_qual=min_qual, **flags)


def _facts(factory):
    o = factory()
    o.assemble()
    return Facts(o), o


CASES_PER_BLOCK = 20


@pytest.mark.parametrize("block", range(SMALL_GRAPH_CASES // CASES_PER_BLOCK))
def test_small_graphs_every_path(block):
    """Cases 0 ... 159 of the family (seed SHK_SMALL_GRAPH_SEED, default 9100; test_oracle.py checks on the CPU what the 160
    reach): each through the default path and through two of the twenty variants, in rotation."""
    tally = {}
    for case, fq, k, min_count, flags in small_graph_cases((block + 1) * CASES_PER_BLOCK):
        if case < block * CASES_PER_BLOCK:
            continue
        factory = _oracle_factory(fq, k, min_count, flags)
        facts, _ = _facts(factory)
        what = f"case {case}"
        check_run(fq, k, min_count, flags, facts, factory, "default", {}, {}, what)
        for i in range(2):
            name, env, kw = VARIANTS[(2 * case + i) % len(VARIANTS)]
            check_run(fq, k, min_count, flags, facts, factory, name, env, kw, what, tally)
    print("markers asserted, block", block, {f"{n}:{'' if p else 'no '}{m}": c for (n, m, p), c in sorted(tally.items())})


WIDE_PARTS = 3                                                      # (a block of 12 inputs in three tests: wide keys take longer)


@pytest.mark.parametrize("part", range(WIDE_PARTS))
@pytest.mark.parametrize("block", range(WIDE_BLOCKS))
def test_small_graphs_wide_keys(block, part):
    """The same structures at keys of two to eight words (k = 63 ... 255): the 24 inputs on which test_oracle.py pins the
    oracle's graph stage with pygraph.py, through the default path and four variants."""
    cases = list(wide_graph_cases(block))
    per = len(cases) // WIDE_PARTS
    for case, fq, k, min_count, flags in cases[part * per:(part + 1) * per]:
        factory = _oracle_factory(fq, k, min_count, flags)
        facts, _ = _facts(factory)
        what = f"wide case {case}"
        check_run(fq, k, min_count, flags, facts, factory, "default", {}, {}, what)
        for name in ("cut", "plan", "device_writer", "shipped"):
            env, kw = VARIANT[name]
            check_run(fq, k, min_count, flags, facts, factory, name, env, kw, what)


# ---- three inputs at the edges the family does not reach ----------------------------------------------------------------
@pytest.mark.parametrize("k", [21, 31])
@pytest.mark.parametrize("m", [255, 256, 257])
def test_chain_records_around_512(m, k):
    """m linear contigs, each its own read: 2 m = 510, 512, 514 chain records around the two limits of 512 — the pinned
    mailbox brings HEADS_SPEC = 512 records with the counters and a second copy the rest; up to PLAN_HEADS = 512 the device
    may plan the emission.  Some reads are exactly k long: a chain whose head node is its tail node."""
    rng = np.random.default_rng(5)
    lens = rng.integers(k, k + 90, m)
    seqs = ["".join(rng.choice(list("ACGT"), int(n))) for n in lens]
    assert k in lens                                                # a one-node chain
    fq = "".join(f"@r{i}\n{s}\n+\n{'I' * len(s)}\n" for i, s in enumerate(seqs)).encode()
    flags = {}
    factory = _oracle_factory(fq, k, 0, flags)
    facts, o = _facts(factory)
    assert facts.ncontigs == m and (o.tips_removed, o.bubbles_removed) == (0, 0)
    what = f"{m} linear contigs"
    ways = [("default", {}), ("plan", {"SHK_DEVICE_PLAN": 1}), ("device_writer_256", {"SHK_DEVICE_WRITER_MIN": 256}),
            ("arrival", {"SHK_ARRIVAL_MIN": 1}), ("seg_cap_600", {"SHK_SEG_CAP": 600, "SHK_SPLIT_LOG": 14}),
            # (the list holds 2 m heads, one per strand, plus the sampled nodes, one in 16384: 514 entries exceed a room of 512)
            ("seg_cap_512", {"SHK_SEG_CAP": 512, "SHK_SPLIT_LOG": 14})]
    for name, env in ways:
        t = check_run(fq, k, 0, flags, facts, factory, name, env, {}, what)
        msg = f"{what} k={k} {name}"
        if name == "plan":
            assert ("collapse_planned_on_device_x1" in t) == (m <= 256), msg
        if name == "device_writer_256":                             # records stay on the device from 2 x 256 of them
            assert ("device_writer_kernels" in t) == (m >= 256), msg
        if name == "arrival":
            assert "collapse_ends_host_clock" in t, msg
        if name == "seg_cap_512" and m == 257:
            assert "collapse_seg_cap_retry_x1" in t, msg


def _plasmid_reads(sizes, k, seed0):
    texts = []
    for j, n in enumerate(sizes):
        g = synth.random_genome(n, seed0 + 10 * k + j)
        codes, quals = synth.sample_reads(g, max(60, n * 30 // 100), 100, 900 + j, circular=True)
        texts.append(synth.to_fastq(codes, quals, prefix=f"c{j}_"))
    return b"".join(texts)


@pytest.mark.parametrize("k", [21, 31])
def test_rings_only(k):
    """No linear chain anywhere: five error-free plasmids.  Every ring an orphan ring (no sampled node: k_orphan_cycles), the
    orphan rings alone outgrowing the room, and every node a splitter (ranks of a few hundred around a ring)."""
    sizes = [k + 2, 40, 64, 200, 333]
    fq = _plasmid_reads(sizes, k, 700)
    flags = {}
    factory = _oracle_factory(fq, k, 1, flags, min_qual=20)
    facts, o = _facts(factory)
    assert facts.ncontigs == 5 and facts.self_links == 5
    assert sorted(len(c) for c in o.contigs()) == sorted(n + k - 1 for n in sizes)
    settings = [("orphans", {"SHK_SPLIT_LOG": 14}), ("orphans_seg_cap1", {"SHK_SPLIT_LOG": 14, "SHK_SEG_CAP": 1}),
                ("all_split_tile1", {"SHK_SPLIT_LOG": 0, "SHK_TILE_ROWS": 1})]
    for name, env in settings:
        for plan in (False, True):
            e = dict(env, **({"SHK_DEVICE_PLAN": 1} if plan else {}))
            nm = name + ("+plan" if plan else "")
            t = check_run(fq, k, 1, flags, facts, factory, nm, e, {}, "rings only", min_qual=20)
            if name == "orphans_seg_cap1":
                assert "collapse_seg_cap_retry_x1" in t, f"rings only k={k} {nm}"
            if plan:
                assert "collapse_planned_on_device_x1" in t, f"rings only k={k} {nm}"


def test_long_chain_many_rank_rounds():
    """One chain of ~6000 nodes with every node a splitter: RANK_HOPS^4 = 4096 < 6000 < RANK_HOPS^5, five rounds of
    k_rank_jump; with SHK_SEG_CAP=1 the ranking is repeated with room for 2 n + 1024 entries."""
    k = 31
    g = synth.random_genome(6000, 4242)
    codes, quals = synth.sample_reads(g, 6000 * 30 // 100, 100, 4243)
    # (uniform starts leave the last few k-mers at either end with a single read: two reads flush with each end keep them solid)
    ends = np.stack([g[:100], g[:100], g[-100:], g[-100:]])
    fq = synth.to_fastq(codes, quals) + synth.to_fastq(ends, np.full(ends.shape, 73, dtype=np.uint8), prefix="e")
    flags = {}
    factory = _oracle_factory(fq, k, 1, flags, min_qual=20)
    facts, o = _facts(factory)
    assert facts.ncontigs == 1 and len(o.contigs()[0]) == 6000
    for name, env in (("all_split", {"SHK_SPLIT_LOG": 0}), ("all_split_seg_cap1", {"SHK_SPLIT_LOG": 0, "SHK_SEG_CAP": 1})):
        t = check_run(fq, k, 1, flags, facts, factory, name, env, {}, "one chain of 6000", min_qual=20)
        assert ("collapse_seg_cap_retry_x1" in t) == (name == "all_split_seg_cap1"), name
