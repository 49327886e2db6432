"""The product on the low-complexity family (tests/lowcomplexity.py): skewed composition, homopolymers, microsatellites, units
that equal their own reverse complement, interrupted repeats, poly-G tails.  Uniform sequence — every other input of the
suite — never caps a pass-1 record at full P, never puts one key into many lanes of a wave, never repeats a k-mer inside a
record, never gives one key more instances than a bucket region holds, and makes no self-loop, no mirror neighbour, no ring of
a handful of nodes and no chain closed onto its own mirror strand.  Everything here is bit-exact against the oracle, which test_lowcomplexity.py pins on the very
same inputs with pygraph.py, cpu_mt.cpp and the host unitig graph.
Run on the MI355X box: pytest -m gpu tests/test_gpu_lowcomplexity.py"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from lowcomplexity import (NARROW_CASES, WIDE_CASES, canonical_counts, classes, composed_counting_input, narrow_cases,
                           wide_cases)
from sparrowhawk_amd import AssemblyHelper, _lib, pack_fastq
from test_gpu_graph_small import VARIANT, VARIANTS, _facts, _oracle_factory, check_run
from test_gpu_parity import product
from test_gpu_unitig_graph import BothPaths
from test_unitig_graph import library_contigs
from util import canonical_int, int_to_words, make_dataset, run_oracle, sorted_table, with_env

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES_PER_BLOCK = 20


# ---- a. the graph stage, every path -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", range(NARROW_CASES // CASES_PER_BLOCK))
def test_low_complexity_graphs_every_path(block):
    """Cases 0 ... 119 of the family: each through the default path (FASTQ text: the device parser packs runs of code 0 and of
    code 3) and through two of the variants of test_gpu_graph_small.py, in rotation — every stage and the variant's markers on
    verbose handles, the two JSON texts on shipped ones."""
    tally = {}
    for case, fq, k, min_count, flags in narrow_cases((block + 1) * CASES_PER_BLOCK)[block * CASES_PER_BLOCK:]:
        factory = _oracle_factory(fq, k, min_count, flags)
        facts, _ = _facts(factory)
        what = f"low-complexity case {case}"
        check_run(fq, k, min_count, flags, facts, factory, "default", {}, {}, what)
        for i in range(2):
            name, env, kw = VARIANTS[(2 * case + i) % len(VARIANTS)]
            check_run(fq, k, min_count, flags, facts, factory, name, env, kw, what, tally)
    print("markers asserted, low-complexity block", block, {f"{n}:{'' if p else 'no '}{m}": c for (n, m, p), c in sorted(tally.items())})


WIDE_PARTS = 3


@pytest.mark.parametrize("part", range(WIDE_PARTS))
def test_low_complexity_wide_keys(part):
    """The 12 wide cases (k = 63 ... 255, stretches of period <= 8 beyond k - 1 + max_n bases inside a read) through the default
    path and four variants."""
    per = WIDE_CASES // WIDE_PARTS
    for case, fq, k, min_count, flags in wide_cases()[part * per:(part + 1) * per]:
        factory = _oracle_factory(fq, k, min_count, flags)
        facts, _ = _facts(factory)
        what = f"low-complexity wide case {case}"
        check_run(fq, k, min_count, flags, facts, factory, "default", {}, {}, what)
        for name in ("cut", "plan", "device_writer", "shipped"):
            env, kw = VARIANT[name]
            check_run(fq, k, min_count, flags, facts, factory, name, env, kw, what)


# ---- c. counting, every mode ------------------------------------------------------------------------------------------------
COUNT_KS = [15, 21, 31, 33, 51, 63, 89, 127, 129, 255]             # W = 1 ... 8, both sides of every word boundary with a kernel instance
COUNT_KNOBS = ["SHK_COUNT_SPLIT", "SHK_COUNT_MODE_GLOBAL", "SHK_COUNT_MERGE", "SHK_PART_P", "SHK_PART_G", "SHK_PART_MAXN",
               "SHK_BATCH_BASES", "SHK_NO_REPARTITION"]


def counting_input(k):
    return composed_counting_input(k, 5000 + k)


def counting_envs(fq):
    n_bases = sum(len(line) for line in fq.split(b"\n")[1::4])
    return [{}, {"SHK_COUNT_SPLIT": 0}, {"SHK_COUNT_MODE_GLOBAL": 1}, {"SHK_COUNT_MERGE": 2}, {"SHK_COUNT_MERGE": 4},
            {"SHK_PART_P": 2}, {"SHK_PART_P": 64}, {"SHK_PART_P": 16384}, {"SHK_PART_G": 1}, {"SHK_PART_MAXN": 5},
            {"SHK_BATCH_BASES": n_bases // 5},                        # (the slice cursors continue across batches)
            {"SHK_NO_REPARTITION": 1, "SHK_PART_P": 2}]


def count_and_compare(fq, k, env, ok_, oc_, histo, total):
    """the product's sorted distinct table, histogram and instance total under `env` against the oracle's; returns timings()"""
    def go():
        h = product(fq, k=k, min_count=0, min_qual=0, assemble=False)
        t = h.timings()                                              # of the preprocess run (distinct() counts again)
        return h, t, sorted_table(*h.distinct())
    h, t, (hk, hc, _) = with_env(env, go)
    try:
        what = f"k={k} env={env}"
        assert hk.shape == ok_.shape, f"{what}: {len(hc)} distinct k-mers, the oracle has {len(oc_)}"
        assert np.array_equal(hk, ok_), what + ": keys differ"
        assert np.array_equal(hc, oc_), what + f": counts differ in {int(np.count_nonzero(hc != oc_))} rows"
        assert np.array_equal(h.histo(), histo), what + ": histogram differs"
        assert h.total_instances == total, what
    finally:
        h.free()
    return t


@pytest.mark.parametrize("k", COUNT_KS)
def test_low_complexity_counting_every_mode(k):
    """One composed input per k (lowcomplexity.composed_counting_input: every unit of the list at 200 and at k + 100 bases in
    a backbone half of which has 15 % G+C, poly-G tails, 0.5 % errors) through every counting mode the environment selects.
    The input caps pass-1 records at every P and holds keys of >= 20 x the median count; for one- and two-word keys the
    dedupe kernel runs exactly where pipeline.hip (run_count_partitions, `split`) says: not in global mode, not with
    SHK_COUNT_SPLIT=0, not with SHK_NO_REPARTITION.
    SHK_PART_WIN is not among the in-process switches: pipeline.hip reads it once per process (part_win, a function-local
    static) — test_low_complexity_counting_forced_window runs it in a process of its own."""
    fq = counting_input(k)
    reached = classes(fq, k)
    assert reached["record_cap"] and reached["heavy"] and reached["homopolymer"] and reached["own_mirror_neighbour"], reached
    o = run_oracle([fq], k=k, min_count=0, min_qual=0)
    ok_, oc_ = o.distinct()
    histo, total = o.histo(), o.total_instances
    base = {name: None for name in COUNT_KNOBS}
    for env in counting_envs(fq):
        t = count_and_compare(fq, k, dict(base, **env), ok_, oc_, histo, total)
        if k <= 63:
            split_on = not ({"SHK_COUNT_SPLIT", "SHK_COUNT_MODE_GLOBAL", "SHK_NO_REPARTITION"} & set(env))
            assert ("count_dedupe_kernel" in t) == split_on, f"k={k} env={env}"
        if "SHK_BATCH_BASES" in env:
            assert t.get("batch_pack_kernel", 0) > 0, f"k={k}: one batch only"


_WINDOW_CHILD = r'''
import os, sys
sys.path.insert(0, os.environ["SHK_ROOT"]); sys.path.insert(0, os.path.join(os.environ["SHK_ROOT"], "tests"))
import numpy as np
from sparrowhawk_amd import AssemblyHelper
from test_gpu_lowcomplexity import COUNT_KS, counting_input
from util import run_oracle, sorted_table
for k in COUNT_KS:
    if k < 31:
        continue
    fq = counting_input(k)
    h = AssemblyHelper.new(k, True, 0, 0, 0, False, False, False, False)
    h.preprocess(fq, None)
    hk, hc, _ = sorted_table(*h.distinct())
    o = run_oracle([fq], k=k, min_count=0, min_qual=0)
    ok_, oc_ = o.distinct()
    assert hk.shape == ok_.shape and np.array_equal(hk, ok_) and np.array_equal(hc, oc_), "k=%d: distinct table differs" % k
    assert np.array_equal(h.histo(), o.histo()) and h.total_instances == o.total_instances, "k=%d: histogram / total differ" % k
    h.free()
    print("k", k, "ok", len(oc_), "distinct", flush=True)
print("WINDOW OK")
'''


@pytest.mark.parametrize("win", [16, 20])
def test_low_complexity_counting_forced_window(win):
    """SHK_PART_WIN = 16 / 20 at every k >= 31 of the counting test, same inputs, same comparison.  The switch is read once
    per process (pipeline.hip, part_win), so setting it between two handles of this process does nothing: a child process
    with the switch in its environment from the start.  Nothing the product reports depends on the window (results never
    do, and no timer or counter names it), so that the child really ran with it rests on reading part_win: the variable's
    name and the three values it accepts are spelled there as they are here.  (No test set this switch before; a windowed minimiser over a
    periodic stretch is where the two window shapes — one block of 16, two of 10 — see the same m-mers throughout.)"""
    env = dict(os.environ, SHK_ROOT=ROOT, SHK_PART_WIN=str(win))
    for name in COUNT_KNOBS:
        env.pop(name, None)
    pr = subprocess.run([sys.executable, "-c", _WINDOW_CHILD], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=300)
    assert pr.returncode == 0 and "WINDOW OK" in pr.stdout, pr.stdout[-1500:] + pr.stderr[-3000:]


# ---- d. a heavy key in partitions that exceed the LDS table ------------------------------------------------------------------
HEAVY_MIN = 100000


@functools.lru_cache(maxsize=None)
def heavy_dataset(k):
    """test_partitions_that_exceed_the_lds_table's error-rich reads with whole poly-G reads and (AC)n reads of 150 bases mixed
    in at random places — at least 1000 of each, and as many as give the poly-G k-mer and each of the two (AC)n k-mers (the
    two phases alternate along a read) HEAVY_MIN instances: 1000 reads of 150 bases hold 1000 (151 - k) k-mers, which is
    below 100 000 from k = 52 on, and half of that per phase of (AC)n.  Returns the FASTQ and the oracle's answer."""
    _g, fq = make_dataset(150000, 12, err=0.02, seed=92)
    lines = fq.decode().split("\n")
    recs = ["\n".join(lines[i:i + 4]) + "\n" for i in range(0, len(lines) - 3, 4)]
    per_read = 151 - k
    n_g = max(1000, -(-HEAVY_MIN // per_read))
    n_ac = max(1000, -(-2 * HEAVY_MIN // per_read))
    qual = "I" * 150
    extra = [f"@g{i}\n{'G' * 150}\n+\n{qual}\n" for i in range(n_g)] + [f"@ac{i}\n{'AC' * 75}\n+\n{qual}\n" for i in range(n_ac)]
    rng = np.random.default_rng(9200 + k)
    where = np.sort(rng.integers(0, len(recs) + 1, len(extra)))
    order = rng.permutation(len(extra))
    out, e = [], 0
    for i in range(len(recs) + 1):
        while e < len(extra) and where[e] == i:
            out.append(extra[order[e]]); e += 1
        if i < len(recs):
            out.append(recs[i])
    fq = "".join(out).encode()
    o = run_oracle([fq], k=k, min_count=0, min_qual=0)
    ok_, oc_ = o.distinct()
    return fq, ok_, oc_, o.histo(), o.total_instances


def _count_of(ok_, oc_, kmer):
    W = ok_.shape[1]
    row = np.flatnonzero(np.all(ok_ == np.array(int_to_words(canonical_int(kmer), W), dtype=np.uint64), axis=1))
    return int(oc_[row[0]]) if len(row) else 0


@pytest.mark.parametrize("mode", ["repartition", "residue", "tiny_buckets", "rescatter"])
@pytest.mark.parametrize("k", [31, 51, 89])
def test_heavy_key_in_partitions_that_exceed_the_lds_table(k, mode):
    """No LDS k-mer table has more than 160 KiB / 8 B = 20 480 slots, so a bucket region — 1.1 table sizes of instances with
    50 % slack (pipeline.hip, run_count_partitions: capb) — stays below 34 000 entries: a key of 100 000 instances fits no
    bucket region, whatever F is chosen.  On uniform reads only SHK_OVF_CAP_PCT=60 made a region overflow.
    What the host loop guarantees with such a key (k_ovf_scatter's bucket is a function of the key alone, so the second
    scatter, with room for the fullest bucket the first one measured + 256, cannot overflow):
      repartition   first scatter overflows in the heavy keys' partitions, the second fits: partitions counted by the bucket
                    path, none re-run by residue classes;
      residue       SHK_NO_REPARTITION: no bucket path at all;
      tiny_buckets  SHK_OVF_MAX_PASSES=1: what overflows is re-run by residue classes — the heavy keys' partitions at least;
      rescatter     as repartition, with every region too small at first.
    What the handle's timings() cannot show: that the heavy keys' partitions were among those handed to the bucket path, and
    that a second scatter ran — no counter depends on either, and the marker assertions below are those of the uniform
    input.  That the first scatter overflows there rests on the arithmetic above and on the oracle's counts asserted first;
    what this test adds beyond it is that the counts come out right with such keys in every mode."""
    fq, ok_, oc_, histo, total = heavy_dataset(k)
    assert len(oc_) > 64 * (6144 if k <= 63 else 3648)                # really more than the LDS tables hold
    heavy = {"poly-G": "G" * k, "(AC)n": ("AC" * k)[:k], "(CA)n": ("CA" * k)[:k]}
    got = {name: _count_of(ok_, oc_, s) for name, s in heavy.items()}
    assert min(got.values()) >= HEAVY_MIN, got
    env = {"SHK_PART_P": 64, "SHK_NO_REPARTITION": None, "SHK_OVF_CAP_PCT": None, "SHK_OVF_MAX_PASSES": None}
    if mode == "residue":
        env["SHK_NO_REPARTITION"] = 1
    if mode == "tiny_buckets":
        env.update(SHK_OVF_CAP_PCT=60, SHK_OVF_MAX_PASSES=1)
    if mode == "rescatter":
        env["SHK_OVF_CAP_PCT"] = 60
    t = count_and_compare(fq, k, env, ok_, oc_, histo, total)
    if mode == "repartition":
        assert t.get("count_repartitioned_x1", 0) > 0 and t.get("count_residue_rerun_x1", 0) == 0, t
    if mode == "residue":
        assert "count_repartitioned_x1" not in t
    if mode == "tiny_buckets":
        assert t.get("count_residue_rerun_x1", 0) > 0, t
    if mode == "rescatter":
        assert t.get("count_residue_rerun_x1", 0) == 0 and t.get("count_repartitioned_x1", 0) > 0, t


# ---- e. the device writer's tie groups ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [21, 31])
def test_device_writer_tie_groups(k):
    """writer_gpu.h orders the contigs by a radix sort on (length, first 16 bases) and settles equal keys by full comparison
    in k_w_ties, an insertion sort whose comment expects runs of two or three, "a few in millions".  Contigs that start in one
    repeat make such runs routinely.  40 loci with a four-allele SNP and bubbles left alone: four branches of 2 k - 1 bases
    that share their first k - 1 — runs of four; ten contigs of one length that begin with the same 20 bases of (AC)n — a
    run of ten.  (All four branches of a locus take the same orientation: the two spellings of a branch differ inside the
    shared k - 1 bases at either end.  The ten end in C, so their mirror spelling starts with G and loses.  At k = 21 the
    shared prefix is 18 bases and each of the ten goes on with a dinucleotide of its own: with 20 shared bases their first
    k-mers are prefix + one base, four nodes for ten contigs, and the ten would fork there instead of being ten contigs.)"""
    rng = np.random.default_rng(3100 + k)

    def rnd(n):
        return "".join(rng.choice(list("ACGT"), n))
    reads = []
    for _ in range(40):
        left, right = rnd(3 * k), rnd(3 * k)
        for b in "ACGT":
            reads += [left + b + right] * 3
    shared = min(20, k - 3)
    own = [a + b for a in "CGT" for b in "ACGT"]                        # (not A: the repeat ends after `shared` bases)
    for i in range(10):
        reads += [("AC" * 10)[:shared] + own[i] + rnd(2 * k + 27 - shared) + "C"] * 3
    order = rng.permutation(len(reads))
    fq = "".join(f"@r{i}\n{reads[j]}\n+\n{'I' * len(reads[j])}\n" for i, j in enumerate(order)).encode()
    flags = dict(no_bubble_collapse=True, no_dead_end_removal=False)
    o = run_oracle([fq], k=k, min_count=1, min_qual=0, **flags)
    o.assemble()
    groups = {}
    for c in o.contigs():
        groups[(len(c), c[:16])] = groups.get((len(c), c[:16]), 0) + 1
    sizes = sorted(groups.values(), reverse=True)
    print("tie groups of the device writer, k", k, ":", sizes[:45])
    assert sizes[0] == 10 and sum(1 for s in sizes if s == 4) >= 30, sizes[:45]       # (the issue's floor: one group of >= 3)

    def run():
        h = AssemblyHelper.new(k, True, 1, 0, 0, False, False, True, False)
        h.preprocess(fq, None)
        h.assemble()
        return h
    host = with_env({"SHK_DEVICE_WRITER_MIN": None}, run)
    dev = with_env({"SHK_DEVICE_WRITER_MIN": 1}, run)
    try:
        assert "device_writer_kernels" in dev.timings() and "device_writer_kernels" not in host.timings()
        assert dev.get_assembly() == o.assembly_json(), "device writer against the oracle"
        assert dev.get_assembly() == host.get_assembly()
    finally:
        host.free(); dev.free()


# ---- f. the device unitig graph ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", range(NARROW_CASES // 40))
def test_device_unitig_graph_on_low_complexity(block):
    """shk_device_unitig_assemble on the chains of the 120 narrow cases, as test_gpu_unitig_graph.py feeds it the random
    graphs: the device text equals the host text (BothPaths), and contigs, count sums and removal counts are the oracle's."""
    from pygraph import PyGraph
    L = BothPaths(_lib.load())
    for case, fq, k, min_count, flags in narrow_cases((block + 1) * 40)[block * 40:]:
        pg = PyGraph(canonical_counts(fq, k), k, min_count)
        o = run_oracle([fq], k=k, min_count=min_count, min_qual=0, **flags)
        o.assemble()
        got, removed = library_contigs(L, pg, k, not flags["no_dead_end_removal"], not flags["no_bubble_collapse"],
                                       drop_mirror_of_short_rings=bool(case % 2))
        want = list(zip(o.contigs(), [int(x) for x in o.contig_kc()]))
        assert got == want, f"case {case}: contigs differ (k={k}, {len(got)} vs {len(want)})"
        assert removed == (o.tips_removed, o.bubbles_removed), f"case {case}"
    assert L.calls == 40


# ---- g. the sharded assembly, one rank ---------------------------------------------------------------------------------------
def test_sharded_graph_one_rank_low_complexity():
    """The loop of test_dist.test_sharded_graph_one_rank_random_graphs (local contraction, stitching, tips / bubbles on the
    unitig graph, emission; a one-rank RCCL communicator in this process) over 60 narrow cases: both JSON texts are the
    oracle's."""
    import torch
    from sparrowhawk_amd.dist import LibComm, sharded_preprocess_rccl
    dev = torch.device("cuda", 0)
    comm = LibComm(0, 1)
    try:
        for case, fq, k, min_count, flags in narrow_cases(60):
            what = f"low-complexity case {case} k={k} min_count={min_count} {flags}"
            bases, seg, nb, nr = pack_fastq(fq, k, 0)
            d_bases = torch.from_numpy(bases.view(np.int32)).to(dev)
            d_seg = torch.from_numpy(seg.view(np.int32)).to(dev)
            torch.cuda.synchronize()
            h = AssemblyHelper.new(k, False, min_count, 0, 0, False, False, flags["no_bubble_collapse"], flags["no_dead_end_removal"])
            try:
                sharded_preprocess_rccl(h, d_bases.data_ptr(), d_seg.data_ptr(), len(seg) - 1, nb, nr, comm)
                h.assemble()
                o = run_oracle([fq], k=k, min_count=min_count, min_qual=0, **flags)
                o.assemble()
                assert h.get_preprocessing_info() == o.preprocessing_json(), what
                assert h.get_assembly() == o.assembly_json(), what
                assert "shard_graph_stitch" in h.timings(), what
            finally:
                h.free()
    finally:
        comm.free()
