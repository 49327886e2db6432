"""The serial chain of a plain one-GPU step (csrc/pipeline.hip): every host wait brings its small results home in one transfer
into the pinned mailbox (CountMail at the wait of pass 2, GraphWords and the first chain records at the wait of rank_chains),
pass 2 follows pass 1 with nothing but k_make_runs in between, and the emission is planned on the device by default with the
text sent through the copy engine.  Every comparison is against the oracle, bit for bit.
Run on the MI355X box: pytest -m gpu tests/test_gpu_step_chain.py"""
import functools

import numpy as np
import pytest

from sparrowhawk_amd import AssemblyHelper, synth
from test_gpu_graph_small import Facts, run_case
from util import compare_all, make_dataset, run_oracle

pytestmark = pytest.mark.gpu

PLANNED = "collapse_planned_on_device_x1"


def _fastq_of(seqs, prefix="r"):
    return "".join(f"@{prefix}{i}\n{s}\n+\n{'I' * len(s)}\n" for i, s in enumerate(seqs)).encode()


def _random_seqs(lens, seed):
    rng = np.random.default_rng(seed)
    return ["".join(rng.choice(list("ACGT"), int(n))) for n in lens]


@functools.lru_cache(maxsize=None)
def _reads_20k(err):
    return make_dataset(20000, 30, err=err, seed=11)[1]


def _factory(fq, k, min_count, min_qual=0):
    return lambda: run_oracle([fq], k=k, min_count=min_count, min_qual=min_qual)


def _facts(factory):
    o = factory()
    o.assemble()
    return Facts(o), o


def _run(fq, k, min_count, env, factory, what, min_qual=0, **kw):
    """One product run under exactly `env`, compared with the oracle: every stage on a verbose handle, the two texts on a quiet
    one (the handle bench.py makes).  Returns (timings, assembly text)."""
    h = run_case(fq, k, min_count, {}, env, min_qual=min_qual, **kw)
    try:
        try:
            if kw.get("shipped"):
                o = factory()
                o.assemble()
                assert h.get_preprocessing_info() == o.preprocessing_json(), "preprocessing info differs"
                assert h.get_assembly() == o.assembly_json(), "assembly differs"
            else:
                compare_all(h, factory(), check_graph=True)
        except AssertionError as e:
            raise AssertionError(f"{what} k={k} min_count={min_count} env={env} {kw}: {e}") from e
        return h.timings(), h.get_assembly()
    finally:
        h.free()


# ---- the read-back of the preprocess ---------------------------------------------------------------------------------------
# (name, k, error rate of the reads, environment)
READBACK = [
    ("k31_clean", 31, 0.0, {}),
    ("k51_two_word_keys", 51, 0.0, {}),
    ("fused_kernel", 31, 0.0, {"SHK_COUNT_SPLIT": 0}),
    ("scattered_rows", 31, 0.0, {"SHK_PART_P": 2}),
    ("no_graph_ranges", 31, 0.0, {"SHK_GRAPH_RANGES": 0}),
    ("errors_left_in", 31, 0.01, {}),
    # every record holds ONE k-mer, the slices are sized for two: the slices of pass 1 overflow, pass 2 has run on a part of
    # the records behind it, and the flags that say so come home with pass 2's read-back — both passes are repeated
    ("slice_overflow", 31, 0.0, {"SHK_PART_MAXN": 1}),
]


@pytest.mark.parametrize("name,k,err,env", READBACK, ids=[c[0] for c in READBACK])
def test_preprocess_readback(name, k, err, env):
    """A 20 kbp genome at 30x: histogram, counts and the assembly through the text entry (verbose handle, every stage) and
    through the packed device entry on a quiet handle, the bench's step."""
    fq = _reads_20k(err)
    factory = _factory(fq, k, 3)
    t, _ = _run(fq, k, 3, env, factory, name)
    tq, _ = _run(fq, k, 3, env, factory, name + " quiet", shipped=True, entry="packed_device")
    print(name, {key: v for key, v in tq.items() if key.endswith("_x1") or key == "partition_retry"})
    if name == "slice_overflow":
        assert "partition_retry" in t and "partition_retry" in tq, (t, tq)
    else:
        assert "partition_retry" not in t and "partition_retry" not in tq, (t, tq)
    if name == "fused_kernel":
        assert "count_dedupe_kernel" not in t
    if name in ("k31_clean", "k51_two_word_keys"):
        assert "count_dedupe_kernel" in t


# ---- stale mailbox ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _datasets_ab():
    """A: one contig at k = 31.  B: another k, another contig count (three linear genomes)."""
    a = _reads_20k(0.0)
    b = b"".join(make_dataset(3000 + 500 * j, 30, seed=40 + j)[1] for j in range(3))
    out = []
    for fq, k in ((a, 31), (b, 21)):
        o = run_oracle([fq], k=k, min_count=3, min_qual=0)
        o.assemble()
        out.append((fq, k, o.preprocessing_json(), o.assembly_json(), Facts(o).ncontigs))
    return out


def _new_handle(k):
    return AssemblyHelper.new(k, False, 3, 0, 0, False, False, False, False)


def test_mailbox_fresh_handles_in_turn():
    """A, B, A in one process, each on a fresh handle: the pooled buffers and the pinned mailbox of the handle before are
    reused, with another k and another number of chain records in them."""
    (fa, ka, pa, aa, na), (fb, kb, pb, ab, nb) = _datasets_ab()
    assert na != nb and ka != kb
    for fq, k, pre, asm in ((fa, ka, pa, aa), (fb, kb, pb, ab), (fa, ka, pa, aa)):
        h = _new_handle(k)
        try:
            h.preprocess(fq)
            h.assemble()
            assert h.get_preprocessing_info() == pre
            assert h.get_assembly() == asm
        finally:
            h.free()


def test_mailbox_two_handles_alive():
    """The same with two handles alive at once, their stages interleaved; then A again on a third while both still live."""
    (fa, ka, pa, aa, _), (fb, kb, pb, ab, _) = _datasets_ab()
    ha, hb, hc = _new_handle(ka), _new_handle(kb), None
    try:
        ha.preprocess(fa)
        hb.preprocess(fb)
        ha.assemble()
        hb.assemble()
        hc = _new_handle(ka)
        hc.preprocess(fa)
        hc.assemble()
        assert (hb.get_preprocessing_info(), hb.get_assembly()) == (pb, ab)
        assert (ha.get_preprocessing_info(), ha.get_assembly()) == (pa, aa)
        assert (hc.get_preprocessing_info(), hc.get_assembly()) == (pa, aa)
    finally:
        for h in (ha, hb, hc):
            if h is not None:
                h.free()


# ---- the emission plan by default ------------------------------------------------------------------------------------------
def _ring_reads(n, seed, prefix):
    g = synth.random_genome(n, seed)
    codes, quals = synth.sample_reads(g, n * 30 // 100, 100, seed + 1, circular=True)
    return synth.to_fastq(codes, quals, prefix=prefix)


def _linear_reads(n, seed, prefix):
    g = synth.random_genome(n, seed)
    codes, quals = synth.sample_reads(g, n * 30 // 100, 100, seed + 1)
    return synth.to_fastq(codes, quals, prefix=prefix)


@functools.lru_cache(maxsize=None)
def _plan_case(name):
    """-> (fastq, k, min_count, min_qual, extra environment, entries, what the oracle must say or None)"""
    text = [dict()]
    if name == "nothing_solid":
        return _reads_20k(0.0), 31, 200, 0, {}, text, lambda f, o: f.ncontigs == 0 and f.n_solid == 0
    if name == "one_linear":
        return _reads_20k(0.0), 31, 3, 0, {}, text, lambda f, o: f.ncontigs == 1 and f.self_links == 0
    if name == "ring_all_sampled":
        return _ring_reads(3000, 61, "c_"), 31, 1, 20, {"SHK_SPLIT_LOG": 0}, text, lambda f, o: f.ncontigs == 1 and f.self_links == 1
    if name == "ring_none_sampled":
        return _ring_reads(3000, 61, "c_"), 31, 1, 20, {"SHK_SPLIT_LOG": 14}, text, lambda f, o: f.ncontigs == 1 and f.self_links == 1
    if name == "ring_and_linear":
        return _ring_reads(3000, 61, "c_") + _linear_reads(4000, 71, "l_"), 31, 2, 20, {}, text, lambda f, o: f.ncontigs == 2 and f.self_links == 1
    if name in ("two_contigs", "seg_cap_retry"):
        env = {"SHK_SEG_CAP": 1, "SHK_TILE_ROWS": 3} if name == "seg_cap_retry" else {}
        return _linear_reads(4000, 71, "a_") + _linear_reads(5000, 81, "b_"), 31, 2, 20, env, text, lambda f, o: f.ncontigs == 2 and f.self_links == 0
    if name == "contigs_256":
        # each read a contig of its own: 512 chain records, the most the device plans
        k = 31
        lens = np.random.default_rng(6).integers(k, k + 90, 256)
        return _fastq_of(_random_seqs(lens, 7)), k, 0, 0, {}, text, lambda f, o: f.ncontigs == 256
    if name == "contigs_300_declined":
        # 300 contigs of 200 bases: 600 chain records, more than the 512 of the plan and of the mailbox — the plan declines, the
        # host plans, and the text already copied is ignored
        return _fastq_of(_random_seqs([200] * 300, 8)), 31, 0, 0, {}, text, lambda f, o: f.ncontigs == 300
    if name == "round0_removes":
        # errors left in at a threshold of one: correction round 0 removes tips and bubbles, the ranking launched behind it
        # returns at once, and the pass — plan, text and all — is repeated on the corrected graph
        return make_dataset(5000, 30, err=0.01, seed=21)[1], 31, 1, 0, {}, text, lambda f, o: o.tips_removed + o.bubbles_removed > 0 and f.ncontigs >= 1
    if name == "packed_entries_quiet":
        return _reads_20k(0.0), 31, 3, 0, {}, [dict(shipped=True, entry="packed_device"), dict(shipped=True, entry="packed_host")], lambda f, o: f.ncontigs == 1
    raise ValueError(name)


PLAN_CASES = ["nothing_solid", "one_linear", "ring_all_sampled", "ring_none_sampled", "ring_and_linear", "two_contigs", "contigs_256",
              "contigs_300_declined", "round0_removes", "seg_cap_retry", "packed_entries_quiet"]


@pytest.mark.parametrize("name", PLAN_CASES)
def test_emission_plan_by_default(name):
    """With nothing set and with SHK_DEVICE_PLAN=0: both equal the oracle and each other; the device plans exactly where the
    oracle's contig count says it can (1 ... 256 contigs: at most 512 chain records, at least one)."""
    fq, k, min_count, min_qual, env, entries, expect = _plan_case(name)
    factory = _factory(fq, k, min_count, min_qual)
    facts, o = _facts(factory)
    assert expect(facts, o), f"{name}: the case is not what it is meant to be (ncontigs {facts.ncontigs}, rings {facts.self_links}, solid {facts.n_solid})"
    for kw in entries:
        t_dev, asm_dev = _run(fq, k, min_count, env, factory, name + " default", min_qual=min_qual, **kw)
        t_host, asm_host = _run(fq, k, min_count, dict(env, SHK_DEVICE_PLAN=0), factory, name + " host plan", min_qual=min_qual, **kw)
        assert asm_dev == asm_host, name
        assert PLANNED not in t_host, (name, kw)
        if 1 <= facts.ncontigs <= 256:
            assert PLANNED in t_dev, (name, kw, facts.ncontigs)
        if facts.ncontigs > 512 or facts.ncontigs == 0:
            assert PLANNED not in t_dev, (name, kw, facts.ncontigs)
        if name == "contigs_300_declined":
            assert PLANNED not in t_dev                              # 600 chain records (a linear contig has one per strand)
        if name == "seg_cap_retry":
            assert "collapse_seg_cap_retry_x1" in t_dev and "collapse_seg_cap_retry_x1" in t_host
