"""The low-complexity family (tests/lowcomplexity.py) on the CPU: the three CPU statements of the SPEC — tests/pygraph.py,
oracle/cpu_mt.cpp and csrc/unitig_graph.cpp — against the oracle on the very inputs test_gpu_lowcomplexity.py sends through
the product, and what those inputs reach.  The GPU tests trust the oracle on this family because of these."""
import numpy as np
import pytest

from lowcomplexity import NARROW_CASES, WIDE_CASES, classes, narrow_cases, record_cap_of, wide_cases, longest_periodic_stretch
from sparrowhawk_amd import _lib
from test_cpu_mt import run_mt
from test_oracle import _pin_case_with_pygraph
from test_unitig_graph import library_contigs
from util import run_oracle

BLOCK = 20


def _block(block):
    return narrow_cases((block + 1) * BLOCK)[block * BLOCK:]


@pytest.mark.parametrize("block", range(NARROW_CASES // BLOCK))
def test_pygraph_pins_the_oracle_on_low_complexity(block):
    """Solid set, counts, adjacency before and after correction, contigs, FASTA, GFA1 and removal counts of the oracle equal
    those of the brute-force Python graph: self-loops, hairpin links, rings of a few nodes and all."""
    stats = dict(tips=0, bubbles=0, rings=0, contigs=0, links=0)
    for case, fq, k, min_count, flags in _block(block):
        _pin_case_with_pygraph(fq, k, min_count, flags, case, stats)
    print("low-complexity campaign, block", block, stats)
    # pygraph's circular unitigs are what lowcomplexity.rings_of counts from the oracle's text (the floors of
    # test_low_complexity_campaign_reaches_every_class rest on that), and every block the GPU campaign runs has one
    from lowcomplexity import rings_of
    n = 0
    for case, fq, k, min_count, flags in _block(block):
        o = run_oracle([fq], k=k, min_count=min_count, min_qual=0, **flags)
        o.assemble()
        n += len(rings_of(o.contigs(), o.gfa1(), k))
    assert stats["rings"] == n and n >= 1, (stats["rings"], n)


@pytest.mark.parametrize("part", range(3))
def test_pygraph_pins_the_oracle_on_low_complexity_wide_keys(part):
    """the 12 cases at k = 63 ... 255, four per test (string k-mers of 255 bases take their time in pygraph.py)"""
    stats = dict(tips=0, bubbles=0, rings=0, contigs=0, links=0)
    for case, fq, k, min_count, flags in wide_cases()[4 * part:4 * part + 4]:
        _pin_case_with_pygraph(fq, k, min_count, flags, case, stats)
    print("low-complexity campaign, wide keys, part", part, stats)


def _cpu_mt_equals_oracle(case, fq, k, min_count, flags):
    o = run_oracle([fq], k=k, min_count=min_count, min_qual=0, **flags)
    m = run_mt(fq, k, min_count, 3, min_qual=0, **flags)
    what = f"case {case} k={k} min_count={min_count} {flags}"
    assert m.total_instances == o.total_instances, what
    assert np.array_equal(m.histo(), o.histo()), what
    mk, mc = m.solid()
    ok_, oc_ = o.solid()
    assert np.array_equal(mk, ok_) and np.array_equal(mc, oc_), what + ": solid sets differ"
    o.assemble()
    assert m.fasta() == o.fasta(), what + ": FASTA differs"


@pytest.mark.parametrize("block", range(NARROW_CASES // BLOCK))
def test_cpu_mt_equals_the_oracle_on_low_complexity(block):
    for case, fq, k, min_count, flags in _block(block):
        _cpu_mt_equals_oracle(case, fq, k, min_count, flags)


def test_cpu_mt_equals_the_oracle_on_low_complexity_wide_keys():
    """cpu_mt.cpp takes keys of one and two words (k <= 63): of the wide cases, those at k = 63."""
    n = 0
    for case, fq, k, min_count, flags in wide_cases():
        if k <= 63:
            _cpu_mt_equals_oracle(case, fq, k, min_count, flags)
            n += 1
    assert n >= 1


@pytest.mark.parametrize("block", range(NARROW_CASES // BLOCK))
def test_host_unitig_graph_equals_the_oracle_on_low_complexity(block):
    """shk_host_unitig_assemble on the uncorrected graph's chains (both strands; short rings on one strand only in alternate
    cases, as the device reports them): the oracle's contigs, count sums and removal counts."""
    from lowcomplexity import canonical_counts
    from pygraph import PyGraph
    L = _lib.load()
    for case, fq, k, min_count, flags in _block(block):
        pg = PyGraph(canonical_counts(fq, k), k, min_count)
        o = run_oracle([fq], k=k, min_count=min_count, min_qual=0, **flags)
        o.assemble()
        got, removed = library_contigs(L, pg, k, not flags["no_dead_end_removal"], not flags["no_bubble_collapse"],
                                       drop_mirror_of_short_rings=bool(case % 2))
        want = list(zip(o.contigs(), [int(x) for x in o.contig_kc()]))
        assert got == want, f"case {case}: contigs differ (k={k}, {len(got)} vs {len(want)})"
        assert removed == (o.tips_removed, o.bubbles_removed), f"case {case}"


def test_predicates_on_hand_made_reads():
    """the class predicates on reads whose classes follow from their spelling"""
    def fq(*reads):
        return "".join(f"@r{i}\n{s}\n+\n{'I' * len(s)}\n" for i, s in enumerate(reads)).encode()
    assert longest_periodic_stretch("T" + "A" * 10 + "C") == 10
    assert longest_periodic_stretch("GG" + "ACGCGT" * 5 + "A") == 31           # period 6, the trailing A continues it
    assert longest_periodic_stretch("C" + "AACCGGTTA" * 4) < 15               # period 9 is beyond 8: a few chance matches only
    assert [record_cap_of(k) for k in (15, 31, 33, 63, 65, 255)] == [47, 31, 63, 63, 63, 63]
    k = 15
    random_read = "ACGTTGCATGCCGATAGCTAGGATCCATTGACCGTA"
    none = classes(fq(random_read), k)
    assert none == dict(homopolymer=False, own_mirror_neighbour=False, record_cap=False, heavy=False)
    assert classes(fq("C" * 20), k)["homopolymer"] and not classes(fq("C" * 20), k)["own_mirror_neighbour"]   # its own successor, not its mirror's
    assert not classes(fq("AC" * 30), k)["homopolymer"]
    at = classes(fq("AT" * 31), k)                                            # 62 = k + 47 bases of period 2
    assert at["own_mirror_neighbour"] and at["record_cap"] and not at["homopolymer"]
    assert not classes(fq("AT" * 30 + "A"), k)["record_cap"]                  # 61 bases: one short
    assert not classes(fq("AC" * 31), k)["own_mirror_neighbour"]              # revcomp GT GT ...: another node
    heavy = classes(fq(*([random_read] + ["G" * 60] * 20)), k)
    assert heavy["heavy"] and heavy["homopolymer"]                            # 920 x CCC...C against a median of 1


def test_low_complexity_campaign_reaches_every_class():
    """test_gpu_lowcomplexity.py sends cases 0 ... 119 (seed SHK_LOW_COMPLEXITY_SEED) and the 12 wide ones through the product.
    That is worth what they reach.  The floors are conditions on the generator, not measurements: if one is missed, the
    generator changes.  A ring here is a circular unitig (lowcomplexity.rings_of: a contig whose ONLY link is onto itself on one
    strand), not any self-linked contig — a homopolymer node with real exits has such a link too.  Floors of the graph
    shapes: a ring in every block of 20 cases that the GPU campaign runs as one test; rings of 2 ... 8 nodes, isolated nodes
    linked to themselves (one node is no ring: v -> v is not simple) and chains closed by their own hairpin links in at least
    six cases each.  The tallies are printed."""
    from lowcomplexity import hairpin_closed_of, isolated_self_loops_of, rings_of
    from test_gpu_graph_small import VARIANTS
    tally = dict(homopolymer=0, own_mirror_neighbour=0, record_cap=0, heavy=0)
    tips = bubbles = self_linked = 0
    ring_nodes, rings_per_block, hairpin_closed = [], [0] * (NARROW_CASES // BLOCK), 0
    cases_with = dict(isolated_self_loop=0, ring_of_2_to_8=0, hairpin_closed=0)
    per_variant = {name: 0 for name, _, _ in VARIANTS}
    for case, fq, k, min_count, flags in narrow_cases():
        for name, hit in classes(fq, k).items():
            tally[name] += hit
        o = run_oracle([fq], k=k, min_count=min_count, min_qual=0, **flags)
        o.assemble()
        tips += o.tips_removed; bubbles += o.bubbles_removed
        gfa = o.gfa1()
        self_linked += sum(1 for l in gfa.split("\n") if l.startswith("L\t") and l.split("\t")[1:3] == l.split("\t")[3:5])
        rings = rings_of(o.contigs(), gfa, k)
        closed = hairpin_closed_of(gfa)
        ring_nodes += rings; rings_per_block[case // BLOCK] += len(rings); hairpin_closed += len(closed)
        cases_with["isolated_self_loop"] += isolated_self_loops_of(o.contigs(), gfa, k) > 0
        cases_with["ring_of_2_to_8"] += any(2 <= n <= 8 for n in rings)
        cases_with["hairpin_closed"] += bool(closed)
        for i in range(2):
            per_variant[VARIANTS[(2 * case + i) % len(VARIANTS)][0]] += 1
    wide = dict(homopolymer=0, own_mirror_neighbour=0, record_cap=0, heavy=0)
    wide_rings = []
    for case, fq, k, min_count, flags in wide_cases():
        for name, hit in classes(fq, k).items():
            wide[name] += hit
        o = run_oracle([fq], k=k, min_count=min_count, min_qual=0, **flags)
        o.assemble()
        wide_rings += rings_of(o.contigs(), o.gfa1(), k)
    print("low-complexity classes, 120 narrow cases:", tally)
    print("oracle, 120 narrow cases:", dict(tips_removed=tips, bubbles_removed=bubbles, contigs_linked_to_themselves=self_linked,
                                            rings=len(ring_nodes), rings_per_block=rings_per_block, ring_nodes=sorted(ring_nodes),
                                            hairpin_closed_chains=hairpin_closed, cases_with=cases_with))
    print("low-complexity classes, 12 wide cases:", wide, "rings (nodes):", sorted(wide_rings))
    print("cases per variant:", per_variant)
    assert min(tally.values()) >= 15, tally
    assert tips >= 1 and bubbles >= 1, (tips, bubbles)
    assert min(rings_per_block) >= 1, rings_per_block
    assert min(cases_with.values()) >= 6, cases_with
    assert len(wide_rings) >= 2, wide_rings
    assert min(per_variant.values()) >= 8, per_variant
    assert wide["record_cap"] >= 4, wide
    assert len(narrow_cases()) == NARROW_CASES and len(wide_cases()) == WIDE_CASES
