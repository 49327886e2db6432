"""shk_preprocess_fasta end to end (SPEC S1a): a FASTA text gives the results of its FASTQ twin — through shk_preprocess and
through the oracle — whatever packer, input form, batch size and counting mode it goes through."""
import gzip
import json

import numpy as np
import pytest

import fasta_cases as fa
from sparrowhawk_amd import AssemblyHelper, synth
from sparrowhawk_amd.helper import ShkError
from util import canonical_int, compare_all, run_oracle, sorted_table, with_env

pytestmark = pytest.mark.gpu

KNOBS = ("SHK_HOST_PARSER", "SHK_FASTA_DEVICE_MIN", "SHK_BATCH_BASES", "SHK_GUNZIP_DEVICE", "SHK_GUNZIP_DEVICE_MIN", "SHK_GUNZIP_DEVICE_WINDOW")


@pytest.fixture(autouse=True)
def knobs(monkeypatch):
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("SHK_FASTA_DEVICE_MIN", "0")             # (the texts here are small: the device packer unless a test says otherwise)


def reads_fasta(genome_len, coverage, seed, err=0.0, width=70, read_len=150):
    g = synth.random_genome(genome_len, seed)
    codes, _ = synth.sample_reads(g, genome_len * coverage // read_len, read_len, seed + 1000, err=err)
    return b"".join(fa.fa(b"r%d" % i, synth.codes_to_str(c).encode(), width) for i, c in enumerate(codes))


def run(data, data2=None, fasta=True, k=31, min_count=3, csize=0, do_bloom=False, do_fit=False, assemble=True, correct=True):
    """a finished helper and what it gave: (info, distinct keys, counts, total_instances, assembly)"""
    h = AssemblyHelper.new(k, True, min_count, 20, csize, do_bloom, do_fit, not correct, not correct)
    (h.preprocess_fasta if fasta else h.preprocess)(data, data2)
    dk, dc, _ = sorted_table(*h.distinct())
    out = [h.get_preprocessing_info(), dk.tolist(), dc.tolist(), h.total_instances]
    if assemble:
        h.assemble()
        out.append(h.get_assembly())
    return h, out


@pytest.fixture(scope="module")
def small():
    """reads of a 30 kbp genome as FASTA (wrapped at 70), their twin, and the results by the device packer"""
    text = reads_fasta(30000, 12, 5, err=0.005)
    twin = fa.fastq_twin(text)
    return text, twin, with_env({"SHK_FASTA_DEVICE_MIN": 0, "SHK_HOST_PARSER": None}, lambda: run(text))


@pytest.mark.parametrize("k,do_fit", [(31, False), (63, False), (31, True)])
def test_fasta_reads_give_the_results_of_their_fastq_twin_and_of_the_oracle(k, do_fit):
    text = reads_fasta(40000, 14, 7 + k, err=0.01)
    twin = fa.fastq_twin(text)
    h, got = run(text, k=k, do_fit=do_fit)
    assert h.timings().get("fasta_device_x1", 0) == 1 and "fasta_host_x1" not in h.timings(), h.timings()
    h2, want = run(twin, fasta=False, k=k, do_fit=do_fit)
    assert got == want
    assert h.states == h2.states                                # the progress strings of the twin's run
    compare_all(h, run_oracle([twin], k=k, min_count=3, min_qual=20, do_fit=do_fit))


def genome_collection():
    core = synth.random_genome(40000, 77)
    rng = np.random.default_rng(78)
    genomes = []
    for j in range(3):
        g = core.copy()
        for p in rng.integers(0, len(g), 25 * j):               # some SNPs
            g[p] = (g[p] + 1 + int(rng.integers(0, 3))) & 3
        if j == 2:
            g = np.concatenate((g[:20000], synth.random_genome(500, 79), g[20000:]))      # one insertion
        s = bytearray(synth.codes_to_str(g).encode())
        s[1000 + 7 * j:1010 + 7 * j] = b"N" * 10
        s[25000:25000 + 50 * (j + 1)] = b"N" * (50 * (j + 1))
        genomes.append(bytes(s))
    return genomes


def test_a_collection_of_genomes_gives_its_compacted_de_bruijn_graph():
    k = 31
    genomes = genome_collection()
    text = b"".join(fa.fa(b"isolate%d some words" % j, s, 60) for j, s in enumerate(genomes))
    h, got = run(text, k=k, min_count=0, correct=False)          # (no tip removal, no bubble popping: the graph of all k-mers)
    assert h.timings().get("fasta_device_x1", 0) == 1, h.timings()
    out = compare_all(h, run_oracle([fa.fastq_twin(text)], k=k, min_count=0, min_qual=20, no_bubble_collapse=True, no_dead_end_removal=True))
    unitigs = [ln for ln in out["outfasta"].split("\n") if ln and not ln.startswith(">")]
    have = set()
    for u in unitigs:
        have.update(canonical_int(u[i:i + k]) for i in range(len(u) - k + 1))
    for s in genomes:
        for part in s.decode().split("N"):
            assert all(canonical_int(part[i:i + k]) in have for i in range(len(part) - k + 1))
    assert "S\t" in out["outgfa"]


def test_plain_gzip_bgzf_two_members_and_a_pair_give_the_same_results(monkeypatch, small):
    monkeypatch.setenv("SHK_GUNZIP_DEVICE_MIN", "65536")
    text, twin, (h0, want) = small
    assert h0.timings().get("fasta_device_x1", 0) == 1
    h, got = run(gzip.compress(text, compresslevel=6))
    t = h.timings()
    assert t.get("gunzip_device_members_x1", 0) == 1 and "gunzip_host_clock" not in t and t.get("fasta_device_x1", 0) == 1, t
    assert got == want
    h, got = run(synth.bgzf_compress(text))
    t = h.timings()
    assert t.get("gunzip_device_members_x1", 0) == 1 and t.get("gunzip_device_bgzf_blocks_x1", 0) > 0 and t.get("fasta_device_x1", 0) == 1, t
    assert got == want
    cut = text.index(b"\n>", len(text) // 2) + 1
    h, got = run(gzip.compress(text[:cut]) + gzip.compress(text[cut:]))      # two members: the host reader
    t = h.timings()
    assert t.get("gunzip_device_members_x1", 0) == 0 and "gunzip_host_clock" in t and t.get("fasta_device_x1", 0) == 1, t
    assert got == want
    for f1, f2 in ((text[:cut], text[cut:]), (text[:cut - 1], gzip.compress(text[cut:])), (gzip.compress(text[:cut], 1), gzip.compress(text[cut:], 9))):
        h, got = run(f1, f2)
        assert h.timings().get("fasta_device_x1", 0) == 2, h.timings()
        assert got == want
    # a damaged gzip file: the host reader's refusal
    z = bytearray(gzip.compress(text))
    z[len(z) // 2] ^= 0x55
    h = AssemblyHelper.new(31, False, 3, 20, 0, False, False, False, False)
    with pytest.raises(ShkError) as e:
        h.preprocess_fasta(bytes(z))
    assert e.value.code == -3


def test_batches_cut_at_headers_and_the_counting_modes(monkeypatch, small):
    text, twin, (h0, want) = small
    assert h0.timings().get("fasta_batches_x1", 0) == 1
    # bulk and chunked give identical results
    h, got = run(text, csize=2)
    assert got == want
    monkeypatch.setenv("SHK_BATCH_BASES", "1024")
    for host in (False, True):
        if host:
            monkeypatch.setenv("SHK_HOST_PARSER", "1")
        h, got = run(text)
        t = h.timings()
        assert t.get("fasta_batches_x1", 0) > 100 and t.get("fasta_host_x1" if host else "fasta_device_x1", 0) > 100, t
        assert ("fasta_device_x1" in t) != host
        assert got == want
        h, got = run(gzip.compress(text))                         # gzip beyond a batch: inflated on the host, cut the same way
        assert h.timings().get("fasta_batches_x1", 0) > 100 and got == want
        # a record beyond a batch
        h = AssemblyHelper.new(31, False, 3, 20, 0, False, False, False, False)
        with pytest.raises(ShkError) as e:
            cut = text.index(b"\n>", 3000) + 1
            h.preprocess_fasta(text[:cut] + fa.fa(b"long", b"ACGT" * 300, 60) + text[cut:])
        assert e.value.code == -1 and "exceeds one batch" in str(e.value), str(e.value)


def test_bloom_mode_stays_within_its_bounds(small):
    """SPEC S4 as tests/test_gpu_parity.py states it for FASTQ: every stored count is the true one or one more, nothing above the
    threshold is lost, the instance total is exact"""
    text, twin, (h0, want) = small
    mc = 3
    h = AssemblyHelper.new(31, True, mc, 20, 0, True, False, False, False)
    h.preprocess_fasta(text)
    assert h.states[1] == "preprocess:bloom:start"
    true = {tuple(r): c for r, c in zip(want[1], want[2])}
    sk, sc = h.solid()
    got = {tuple(r): int(c) for r, c in zip(sk.tolist(), sc.tolist())}
    for key, c in got.items():
        assert key in true and c in (true[key], true[key] + 1), (key, c, true.get(key))
    assert {key for key, c in true.items() if c > mc} <= set(got) <= {key for key, c in true.items() if c >= mc}
    assert h.total_instances == want[3]


def test_the_switches_choose_the_packer(monkeypatch, small):
    text, twin, (h0, want) = small
    monkeypatch.setenv("SHK_HOST_PARSER", "1")
    h, got = run(text)
    t = h.timings()
    assert t.get("fasta_host_x1", 0) == 1 and "fasta_device_x1" not in t and got == want, t
    monkeypatch.delenv("SHK_HOST_PARSER")
    # the minimum size: below it the host packer, above it — by default too — the device packer
    monkeypatch.setenv("SHK_FASTA_DEVICE_MIN", str(len(text) + 1))
    h, got = run(text)
    assert h.timings().get("fasta_host_x1", 0) == 1 and got == want
    monkeypatch.setenv("SHK_FASTA_DEVICE_MIN", str(len(text)))
    assert run(text)[0].timings().get("fasta_device_x1", 0) == 1
    monkeypatch.delenv("SHK_FASTA_DEVICE_MIN")
    big = text * (1 + (8 << 20) // len(text))                   # above any default that is not "never"
    h = AssemblyHelper.new(31, False, 3, 20, 0, False, False, False, False)
    h.preprocess_fasta(big)
    assert h.timings().get("fasta_device_x1", 0) == 1, h.timings()


def test_the_contract_and_the_errors(small):
    text, twin, (h0, want) = small
    h2, want2 = run(twin, fasta=False)
    assert h0.states == h2.states and want == want2
    # chunked mode posts a mark every chunk_size records: the same records; the percentages are bytes of another text
    hc, _ = run(text, csize=500)
    hq, _ = run(twin, fasta=False, csize=500)
    strip = lambda states: [s.rsplit(":", 1)[0] if s.startswith("preprocess:chunked:loop:") else s for s in states]      # noqa: E731
    assert strip(hc.states) == strip(hq.states) and sum(s.startswith("preprocess:chunked:loop:") for s in hc.states) > 3
    with pytest.raises(ShkError) as e:
        h0.preprocess_fasta(text)
    assert e.value.code == -2
    # a text with no record at all behaves as an empty FASTQ text does
    def outcome(data, fasta):
        h = AssemblyHelper.new(31, False, 3, 20, 0, False, False, False, False)
        try:
            (h.preprocess_fasta if fasta else h.preprocess)(data)
            return json.loads(h.get_preprocessing_info())["nkmers"], h.states
        except ShkError as err:
            return err.code
    assert outcome(b"", True) == outcome(b"", False) and outcome(b"\n\n", True) == outcome(b"", False)
    # refusals: sequence in front of the first header, in either file; FASTA through shk_preprocess as before
    for f1, f2 in ((b"ACGT\n" + text, None), (text, b"ACGT\n" + text), (twin, None)):
        h = AssemblyHelper.new(31, False, 3, 20, 0, False, False, False, False)
        with pytest.raises(ShkError) as e:
            h.preprocess_fasta(f1, f2)
        assert e.value.code == -3 and "FASTA" in str(e.value), str(e.value)
    h = AssemblyHelper.new(31, False, 3, 20, 0, False, False, False, False)
    with pytest.raises(ShkError) as e:
        h.preprocess(text)
    assert e.value.code == -3
