"""The sharded assembly (csrc/shard_graph.h and the steps of Pipeline::shard_assemble in csrc/pipeline.hip) on the adversarial
small graphs of test_oracle._random_graph_case, through every path of it that the environment can select: the sharded twin
of test_gpu_graph_small.py.  One rank in this process, and 2, 3 and 4 ranks on the one GPU with their bytes through
tests/mock_rccl; handles with stage inspection and shipped ones (quiet, no SHK_STAGE_TIMERS, no SHK_KEEP_STAGES).  Every
rank of every run must end with the oracle's two texts, byte for byte.
Which case meets which variant is fixed by the functions below; test_oracle.py checks on the CPU what that reaches.
Run on the MI355X box: pytest -m gpu tests/test_gpu_shard_graph_small.py"""
import functools
import json
import os
import tempfile
import time

import numpy as np
import pytest

from test_oracle import SMALL_GRAPH_CASES, small_graph_cases, wide_graph_cases, WIDE_BLOCKS, WIDE_PER_BLOCK
from test_dist import launch, mock_rccl_library, _write_cases
from util import run_oracle, with_env

pytestmark = pytest.mark.gpu

# name, environment, handle keywords.  Only knobs that the sharded path reads: SHK_GRAPH_RANGES, SHK_GRAPH_LDS_SLOTS (build_graph:
# `ranges` requires !sh_active_), SHK_DEVICE_PLAN and SHK_ARRIVAL_* (collapse(), which the sharded assembly never calls) are
# left out; SHK_DEVICE_WRITER_MIN is read by sh_emit.
DEFAULT = ("default", {}, {})
_ALL_DEVICE = {"SHK_UNITIG_DEVICE": 1, "SHK_DEVICE_WRITER_MIN": 1}
VARIANTS = [
    ("tile1_all_split", {"SHK_TILE_ROWS": 1, "SHK_SPLIT_LOG": 0}, {}),          # tile edges at every row, rank edges among them
    ("tile3_no_split", {"SHK_TILE_ROWS": 3, "SHK_SPLIT_LOG": 14}, {}),          # no sampled node: orphan rings inside a rank
    ("tile17", {"SHK_TILE_ROWS": 17, "SHK_SPLIT_LOG": 3}, {}),
    ("seg_cap1", {"SHK_SEG_CAP": 1}, {}),                                       # the retry, chain records staying on the device
    ("seg_cap8_all_split", {"SHK_SEG_CAP": 8, "SHK_SPLIT_LOG": 0, "SHK_TILE_ROWS": 64}, {}),
    ("tiny_parts", {"SHK_GP_ROWS": 16}, {}),                                    # thousands of graph partitions, cut from the GLOBAL count
    ("regroup", {"SHK_REGROUP_ROWS": 1}, {}),                                   # rows renumbered in front of the cross-rank exchange
    ("no_scan", {"SHK_REGROUP_ROWS": 0, "SHK_KEEP_SCAN": 0}, {}),
    ("unitig_device", {"SHK_UNITIG_DEVICE": 1}, {}),
    ("unitig_device_host_walk", {"SHK_UNITIG_DEVICE": 1, "SHK_UNITIG_CHAINS_DEVICE": 0}, {}),
    ("all_device", dict(_ALL_DEVICE), {}),
    ("all_device_retry", dict(_ALL_DEVICE, SHK_SEG_CAP=1, SHK_TILE_ROWS=3), {}),
    ("shipped", {}, dict(shipped=True)),
    ("shipped_all_device", dict(_ALL_DEVICE), dict(shipped=True)),
    ("shipped_retry", {"SHK_SEG_CAP": 1}, dict(shipped=True)),
]
ALL = [DEFAULT] + VARIANTS
# every knob a variant turns: a run that does not name one runs with it unset
KNOBS = sorted({k for _, env, _ in VARIANTS for k in env})
INSPECTION = ("SHK_KEEP_STAGES", "SHK_STAGE_TIMERS")                # what conftest.py sets for every test; read per handle

WORLDS = (2, 3, 4)
CASES_PER_BLOCK = 20
PORT0 = 29860                                                       # + world


# ---- which case meets which variant (pure: test_oracle.py imports these) ------------------------------------------------
def one_rank_variants(case):
    """A small-graph case on one rank: the default path and two of the fifteen variants, in rotation."""
    return [DEFAULT] + [VARIANTS[(2 * case + i) % len(VARIANTS)] for i in range(2)]


def wide_variants(case):
    """A wide-key case on one rank: two of the sixteen rows (the default path among them), in rotation.  (From row 6: four of
    the 24 inputs have no solid k-mer at all — a sharded run of nothing, worth having — and from row 0 they would take a
    block's only run of a row whose marker needs rows or contigs.  test_oracle.py checks what each block reaches.)"""
    return [ALL[(2 * case + i + 6) % len(ALL)] for i in range(2)]


def world_picks(world):
    """What one launch of `world` ranks carries: every fourth small-graph case from an offset of its own, four wide-key cases,
    each with its variant in rotation (44 cases over 16 rows: every row two or three times).  [(what, kind, case, variant)]"""
    off = world - WORLDS[0]
    picks = [("case %d" % c, "small", c) for c in range(off, SMALL_GRAPH_CASES, 4)]
    picks += [("wide case %d" % c, "wide", c) for c in range(off, WIDE_BLOCKS * WIDE_PER_BLOCK, 6)]
    return [(what, kind, c, ALL[(j + 5 * off) % len(ALL)]) for j, (what, kind, c) in enumerate(picks)]


@functools.lru_cache(maxsize=None)
def _wide_cases():
    return {cs[0]: cs for block in range(WIDE_BLOCKS) for cs in wide_graph_cases(block)}


def the_case(kind, c):
    """(case, fastq, k, min_count, flags)"""
    return small_graph_cases(c + 1)[c] if kind == "small" else _wide_cases()[c]


class Facts:
    """What the marker conditions may know about a case: the ORACLE's answer, never the product's."""
    def __init__(self, o):
        self.pre, self.asm = o.preprocessing_json(), o.assembly_json()
        ref = json.loads(self.asm)
        self.ncontigs = ref["ncontigs"]
        self.nkmers = json.loads(self.pre)["nkmers"]                 # solid k-mers: the nodes of the graph as built
        self.removed = o.tips_removed + o.bubbles_removed
        links = [l.split("\t") for l in ref["outgfa"].split("\n") if l.startswith("L\t")]
        self.self_links = sum(1 for f in links if f[1] == f[3] and f[2] == f[4])        # rings: a contig linked to itself on one strand
        self.other_links = sum(1 for f in links if f[1] != f[3])


@functools.lru_cache(maxsize=None)
def facts_of(kind, c):
    """Computed once per case and session, shared by every test that runs the case, never changed."""
    case, fq, k, min_count, flags = the_case(kind, c)
    o = run_oracle([fq], k=k, min_count=min_count, min_qual=0, **flags)
    o.assemble()
    return Facts(o)


# ---- path markers -------------------------------------------------------------------------------------------------------
# All but one (shard_graph_stitch, a stage timer: it tells a shipped handle from the others) are counters that times_.add
# records on every handle, with or without stage timers: checked on shipped runs too.
# Each condition comes from the code and from the oracle's facts; where it is per rank, from the rank's own row count
# (n_solid_local, which the ranks' sum pins to the oracle's nkmers).
#
# retry under SHK_SEG_CAP=1 — the sharded assembly corrects on the UNITIG graph, so rank_chains(rings=false) ranks the graph
# as built, and tips and bubbles go as whole unitigs: every contig of the oracle holds at least one unitig of that graph, and
# different contigs different ones.  A unitig has nodes on at least one rank, and there it brings at least one entry of that
# rank's splitter list: a head per strand of a local chain (k_succ_split: no simple predecessor, a neighbour with the XREF
# bit ends the chain), a sampled node, or the orphan-ring entry (k_orphan_cycles).  So the ranks' lists hold at least
# `ncontigs` entries together, and with ncontigs > world some rank holds two: more than the room of one (flag 4 from
# k_local_frag, or 2 from k_orphan_cycles), and seg_cap64 = 1 < cap_all: that rank repeats the pass.
def _retry_somewhere_seg_cap1(f, world):
    return f.ncontigs > world


# retry under SHK_SEG_CAP=8 SHK_SPLIT_LOG=0 — no node-level correction in the sharded assembly: k_row_starts sets every row
# alive, node_sampled with mask 0 makes every alive oriented node a splitter, so a rank's list holds exactly 2 x its rows
# and k_local_frag calls the pass off (*n_spl_p > seg_cap) where that is above 8.
def _retry_here_all_split(n_local):
    return 2 * n_local > 8


REQUIRED = ("cut", "regrouped", "not_regrouped", "retry_seg_cap1", "retry_all_split", "unitig_device", "writer_device", "no_stage_timers")


def reachable(env, f, world, shipped=False):
    """The REQUIRED keys that a run of this environment on this case is CERTAIN to tally, by the oracle alone (for the per-rank
    conditions: some rank holds at least nkmers / world rows).  test_oracle.py checks that every test reaches every key."""
    keys = {"cut"}
    if shipped: keys.add("no_stage_timers")
    if env.get("SHK_REGROUP_ROWS") == 1 and f.nkmers > 0: keys.add("regrouped")
    if env.get("SHK_REGROUP_ROWS") == 0: keys.add("not_regrouped")
    if env.get("SHK_SEG_CAP") == 1 and _retry_somewhere_seg_cap1(f, world): keys.add("retry_seg_cap1")
    if env.get("SHK_SEG_CAP") == 8 and _retry_here_all_split(-(-f.nkmers // world)): keys.add("retry_all_split")
    if env.get("SHK_UNITIG_DEVICE") == 1: keys.add("unitig_device")
    if env.get("SHK_DEVICE_WRITER_MIN") == 1 and f.ncontigs >= 1: keys.add("writer_device")
    return keys


def check_markers(name, env, f, ranks, msg, tally, shipped=False):
    """ranks: [(timings, n_solid_local)] of one run, one entry per rank.  Asserts what is certain, tallies the rest."""
    world = len(ranks)

    def met(key):
        tally[key] = tally.get(key, 0) + 1
    for r, (t, n_local) in enumerate(ranks):
        m = f"{msg} rank {r} of {world} (rows {n_local}): "
        # build_graph: `if (n || sh_active_)`, and `ranges` requires !sh_active_: the partitions are cut, on every rank, rows or not
        assert t.get("graph_partitions_cut_x1") == 1, m + "graph_partitions_cut_x1 missing"
        assert "graph_partitions_from_counting_x1" not in t, m + "graph_partitions_from_counting_x1 present"
        met("cut")
        # sh_stitch: `if (ts.on()) times_.add("shard_graph_stitch", ...)`, an EvTimer, on with stage_timers_ alone (set_verbose, or
        # SHK_STAGE_TIMERS when the handle is made): a shipped handle must not have it — that it IS shipped is checked here
        assert ("shard_graph_stitch" in t) == (not shipped), m + "shard_graph_stitch " + ("present on a shipped handle" if shipped else "missing")
        if shipped: met("no_stage_timers")
        # build_graph: `n && (regroup_env == 1 || (regroup_env == 2 && rows_scattered_))`
        if env.get("SHK_REGROUP_ROWS") == 1:
            assert ("graph_rows_regrouped_x1" in t) == (n_local > 0), m + "graph_rows_regrouped_x1"
            if n_local > 0: met("regrouped")
        elif env.get("SHK_REGROUP_ROWS") == 0:
            assert "graph_rows_regrouped_x1" not in t, m + "graph_rows_regrouped_x1 present"
            met("not_regrouped")
        elif "graph_rows_regrouped_x1" in t:
            met("(tally) regrouped by the library's own choice")
        if env.get("SHK_SEG_CAP") == 8 and _retry_here_all_split(n_local):
            assert "collapse_seg_cap_retry_x1" in t, m + "collapse_seg_cap_retry_x1 missing"
            met("retry_all_split")
        # sh_unitig_graph: the device twin declines only where the device has no room
        if env.get("SHK_UNITIG_DEVICE") == 1:
            assert t.get("shard_graph_unitig_device_x1") == 1 and "shard_graph_unitig_device_declined_x1" not in t, m + "shard_graph_unitig_device_x1"
            met("unitig_device")
            if "shard_graph_unitig_chains_device_x1" in t: met("(tally) unitig chains walked on the device")
        elif "shard_graph_unitig_device_x1" in t:
            met("(tally) unitig graph on the device by the library's own choice")
        # sh_emit: want_json (always, from shk_assemble) && text_bytes && n_contigs >= SHK_DEVICE_WRITER_MIN, the same on every rank
        if env.get("SHK_DEVICE_WRITER_MIN") == 1 and f.ncontigs >= 1:
            assert t.get("shard_writer_device_x1") == 1 and "shard_writer_device_declined_x1" not in t, m + "shard_writer_device_x1"
            met("writer_device")
        elif f.ncontigs < 20000:                                     # (its default)
            assert "shard_writer_device_x1" not in t, m + "shard_writer_device_x1 present"
    if env.get("SHK_SEG_CAP") == 1:
        n_retry = sum("collapse_seg_cap_retry_x1" in t for t, _ in ranks)
        if _retry_somewhere_seg_cap1(f, world):
            assert n_retry >= 1, f"{msg}: no rank repeated the ranking (ncontigs {f.ncontigs}, {world} ranks)"
            met("retry_seg_cap1")
        elif n_retry:
            met("(tally) retry under SHK_SEG_CAP=1 with ncontigs <= world")
    elif "SHK_SEG_CAP" not in env and any("collapse_seg_cap_retry_x1" in t for t, _ in ranks):
        met("(tally) retry with the default room")


def run_env(env, shipped):
    """Exactly the variant's environment: every other knob of the table unset, the inspection variables unset for a shipped
    handle (else as conftest.py left them)."""
    e = {name: None for name in KNOBS}
    e.update(env)
    if shipped:
        e.update({name: None for name in INSPECTION})
    return e


# ---- one rank, in this process ------------------------------------------------------------------------------------------
def run_one_rank(comm, fq, k, min_count, flags, env, shipped=False):
    """One product run on the one-rank communicator: the handle is made, fed and assembled under run_env, the environment
    restored.  Returns (preprocessing text, assembly text, timings, rows)."""
    import torch
    from sparrowhawk_amd import AssemblyHelper, pack_fastq
    from sparrowhawk_amd.dist import sharded_preprocess_rccl

    def go():
        dev = torch.device("cuda", 0)
        bases, seg, nb, nr = pack_fastq(fq, k, 0)
        d_bases = torch.from_numpy(bases.view(np.int32)).to(dev)
        d_seg = torch.from_numpy(seg.view(np.int32)).to(dev)
        torch.cuda.synchronize()
        h = AssemblyHelper.new(k, not shipped, min_count, 0, 0, False, False, bool(flags.get("no_bubble_collapse")),
                               bool(flags.get("no_dead_end_removal")))
        try:
            sharded_preprocess_rccl(h, d_bases.data_ptr(), d_seg.data_ptr(), len(seg) - 1, nb, nr, comm)
            h.assemble()
            return h.get_preprocessing_info(), h.get_assembly(), h.timings(), h.n_solid
        finally:
            h.free()
    return with_env(run_env(env, shipped), go)


def check_one_rank(comm, kind, c, variants, tally, runs):
    case, fq, k, min_count, flags = the_case(kind, c)
    f = facts_of(kind, c)
    for name, env, kw in variants:
        msg = f"{kind} case {case} k={k} min_count={min_count} flags={flags} variant={name} env={env} {kw}"
        pre, asm, t, n_local = run_one_rank(comm, fq, k, min_count, flags, env, **kw)
        assert pre == f.pre, msg + ": preprocessing info differs"
        assert asm == f.asm, msg + ": assembly differs"
        assert n_local == f.nkmers, msg
        check_markers(name, env, f, [(t, n_local)], msg, tally, **kw)
        runs[name] = runs.get(name, 0) + 1


def _close(what, tally, runs, t0):
    print(what, "runs", dict(sorted(runs.items())), "markers", dict(sorted(tally.items())), "seconds", round(time.time() - t0, 1))
    missing = [key for key in REQUIRED if not tally.get(key)]
    assert not missing, f"{what}: asserted markers never met: {missing}"


@pytest.mark.parametrize("block", range(SMALL_GRAPH_CASES // CASES_PER_BLOCK))
def test_sharded_small_graphs_one_rank(block):
    """Cases 0 ... 159 of the family (seed SHK_SMALL_GRAPH_SEED, default 9100), 20 per block: each through the default path
    and through two of the fifteen variants, in rotation."""
    from sparrowhawk_amd.dist import LibComm
    tally, runs, t0 = {}, {}, time.time()
    comm = LibComm(0, 1)
    try:
        for c in range(block * CASES_PER_BLOCK, (block + 1) * CASES_PER_BLOCK):
            check_one_rank(comm, "small", c, one_rank_variants(c), tally, runs)
    finally:
        comm.free()
    _close(f"one rank, block {block}:", tally, runs, t0)


@pytest.mark.parametrize("block", range(WIDE_BLOCKS))
def test_sharded_small_graphs_one_rank_wide_keys(block):
    """The same structures at keys of two to eight words (k = 63 ... 255): the 24 inputs on which test_oracle.py pins the
    oracle's graph stage, each through two of the sixteen rows."""
    from sparrowhawk_amd.dist import LibComm
    tally, runs, t0 = {}, {}, time.time()
    comm = LibComm(0, 1)
    try:
        for case, *_ in wide_graph_cases(block):
            check_one_rank(comm, "wide", case, wide_variants(case), tally, runs)
    finally:
        comm.free()
    _close(f"one rank, wide keys, block {block}:", tally, runs, t0)


# ---- several ranks ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", WORLDS)
def test_sharded_small_graphs_several_ranks(world):
    """2, 3 and 4 ranks on the one GPU, bytes through tests/mock_rccl (plain for 2 ranks, at its most hostile for 3 and 4;
    MOCK_RCCL_JITTER overrides), ONE launch of 44 cases, each with its variant's environment set by the worker on every rank
    (dist_worker.py, "env").  At 4 ranks a genome of 300 bases leaves ranks with few rows or none."""
    picks = world_picks(world)
    cases = []
    for what, kind, c, (name, env, kw) in picks:
        case, fq, k, min_count, flags = the_case(kind, c)
        shipped = bool(kw.get("shipped"))
        cases.append((fq, dict(k=k, min_count=min_count, min_qual=0, verbose=not shipped, timings=True, env=run_env(env, shipped), **flags)))
    os.environ["SHK_RCCL_LIBRARY"] = mock_rccl_library()
    jitter_was = os.environ.get("MOCK_RCCL_JITTER")
    if jitter_was is None:
        os.environ["MOCK_RCCL_JITTER"] = "1" if world >= 3 else "0"
    t0 = time.time()
    try:
        with tempfile.TemporaryDirectory() as d:
            cfgp = _write_cases(d, cases)
            out = os.path.join(d, "res")
            launch(world, ["rccl_many", out, cfgp], PORT0 + world, timeout=420 + 3 * len(cases))
            res = [json.load(open(f"{out}.{r}")) for r in range(world)]
    finally:
        os.environ.pop("SHK_RCCL_LIBRARY", None)
        if jitter_was is None:
            os.environ.pop("MOCK_RCCL_JITTER", None)
    t_launch = time.time() - t0
    tally, runs = {}, {}
    assert all(len(res[r]) == len(picks) for r in range(world))
    fewest_rows = None
    for i, (what, kind, c, (name, env, kw)) in enumerate(picks):
        f = facts_of(kind, c)
        msg = f"{what} variant={name} env={env} {kw} on {world} ranks"
        for r in range(world):
            assert "error" not in res[r][i], (msg, r, res[r][i])
            assert res[r][i]["pre"] == f.pre, msg + f": preprocessing info differs on rank {r}"
            assert res[r][i]["asm"] == f.asm, msg + f": assembly differs on rank {r}"
        rows = [res[r][i]["n_solid_local"] for r in range(world)]
        assert sum(rows) == f.nkmers, (msg, rows)
        if f.nkmers:
            fewest_rows = min(rows) if fewest_rows is None else min(fewest_rows, min(rows))
        check_markers(name, env, f, [(res[r][i]["timings"], rows[r]) for r in range(world)], msg, tally, **kw)
        runs[name] = runs.get(name, 0) + 1
    print("fewest rows on a rank, of the cases with a solid k-mer:", fewest_rows, "launch seconds", round(t_launch, 1))
    assert set(runs) == {name for name, _, _ in ALL} and min(runs.values()) >= 2, runs
    _close(f"{world} ranks:", tally, runs, t0)
