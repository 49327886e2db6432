"""No result may depend on what a block of the device pool held before.

A block of the pool (csrc/block_cache.h, csrc/device_mem.hip) is never cleared: a request is rounded up to 4 KiB, a cached
block of up to bytes + bytes/2 + 1 MiB may be handed out in its place, so almost every buffer ends in a tail nobody wrote and
starts with what its previous user left.  Every other test sees ONE accidental history of the pool — often freshly zeroed
driver memory.  Here the pool's contents are an input: with shk_debug_pool_fill on, every block is filled with a chosen word
when it is handed out, and every device entry point runs its small edge catalogue under three words:

  0x00000000   stale memory that looks like cleared memory: the lucky case
  0xFFFFFFFF   looks like the tables' empty-slot marker: hides a table that was never initialised, exposes a counter that was not
  0x00000001   small, valid-looking counts, flags and offsets: the word most likely to give a silently wrong answer

The reference of every test is the one the existing test of that entry point uses — the oracle, the SPEC packers, zlib, the
host twin, the golden file — never another run of the product; catalogues and comparers are imported from those tests.  Every
test asserts that shk_debug_pool_filled_bytes() grew while it ran: a test that ran unfilled fails.  The mode serialises the
handles of a process (the fill waits for the whole device): it shows a dependence on stale data, it does not show races.
Run on the MI355X box: pytest -m gpu tests/test_gpu_pool_fill.py"""
import ctypes as C
import functools
import gzip
import json
import os
import tempfile
import zlib

import numpy as np
import pytest

import bgzf_write_cases as bw
import deflate_catalogue as dc
import deflate_writer as dw
import fasta_cases as fa
import fastq_cases as fc
import test_gpu_bgzf_write as bgz
import test_gpu_deflate_streams as ds
import test_gpu_graph_small as gs
import test_gpu_lowcomplexity as lc
import test_gpu_shard_fastq as sq
import test_gpu_shard_graph_small as sgs
import test_gpu_text_writer as tw
import test_gpu_unitig_graph as ug
from sparrowhawk_amd import AssemblyHelper, pack_fastq, synth
from test_bgzf_write_host import host_file
from test_dist import _oracle_jsons, _write_cases, launch, mock_rccl_library
from test_fastq_cases import assert_same_batch, host_pack, joined
from test_gpu_fasta_pack import device_pack as device_pack_fasta
from test_gpu_fastq_pack import SHK_E_PARSE, device_pack as device_pack_fastq
from test_gpu_shard_fasta import NONE, device_first, device_last, host_first, host_last
from test_gpu_unitig_chains import both as chains_device_equals_host
from test_oracle import small_graph_cases, wide_graph_cases, WIDE_BLOCKS
from unitig_chains_cases import KS, Builder, random_case
from util import compare_all, make_dataset, revcomp, run_oracle

pytestmark = pytest.mark.gpu

WORDS = [0x00000000, 0xFFFFFFFF, 0x00000001]


class Fill:
    def __init__(self, lib, word):
        self.lib, self.word, self.start = lib, word, lib.shk_debug_pool_filled_bytes()

    def filled(self):
        return self.lib.shk_debug_pool_filled_bytes() - self.start

    def check(self, what):
        """the closing assertion of every test: blocks were filled while it ran"""
        n = self.filled()
        print("pool fill 0x%08x: %s: %d bytes filled" % (self.word, what, n))
        assert n > 0, what + ": no block of the pool was filled: the test ran unfilled"


@pytest.fixture(params=WORDS, ids=["%08x" % w for w in WORDS])
def fill(request, lib, monkeypatch):
    """The fill switched on with the word of this run; the previous state comes back afterwards."""
    monkeypatch.delenv("SHK_HOST_PARSER", raising=False)             # (as test_gpu_fastq_pack.py: the device parser is what runs)
    was = lib.shk_debug_pool_fill(1, request.param)
    try:
        yield Fill(lib, request.param)
    finally:
        lib.shk_debug_pool_fill(was, request.param if was else 0)


# ---- the mode itself ------------------------------------------------------------------------------------------------------
def probe(lib, n):
    first, last, block = C.c_uint32(0), C.c_uint32(0), C.c_size_t(0)
    assert lib.shk_debug_pool_probe(n, C.byref(first), C.byref(last), C.byref(block)) == 0, n
    return first.value, last.value, block.value


def test_probe(lib, fill):
    """First and last word of the block handed out for 1, 4095, 4096, 4097 bytes and 1 MiB + 1: the WHOLE rounded block is
    filled.  Then a larger block reused: a block of 3 MiB goes back filled with another word, and the request for 2 MiB + 1
    that takes it over finds this run's word in its last word, far behind the bytes asked for."""
    for n in (1, 4095, 4096, 4097, (1 << 20) + 1):
        first, last, block = probe(lib, n)
        assert (first, last) == (fill.word, fill.word), (n, hex(first), hex(last))
        assert block >= n and block % 4096 == 0, (n, block)
    lib.shk_release_cached_memory()                                 # (nothing cached: the 3 MiB block is the one that is found)
    other = fill.word ^ 0x5A5A5A5A
    lib.shk_debug_pool_fill(1, other)
    first, last, block = probe(lib, 3 << 20)
    assert (first, last, block) == (other, other, 3 << 20)
    lib.shk_debug_pool_fill(1, fill.word)
    before = fill.filled()
    first, last, block = probe(lib, (2 << 20) + 1)
    assert block == 3 << 20, block                                   # the cached, larger block
    assert (first, last) == (fill.word, fill.word), (hex(first), hex(last))
    assert fill.filled() - before == 3 << 20                        # counted with its whole size
    fill.check("probe")


def test_the_switch_returns_the_previous_state_and_off_fills_nothing(lib, fill):
    assert lib.shk_debug_pool_fill(0, 0) == 1
    n = lib.shk_debug_pool_filled_bytes()
    probe(lib, 4096)
    assert lib.shk_debug_pool_filled_bytes() == n
    assert lib.shk_debug_pool_fill(1, fill.word) == 0
    assert probe(lib, 4096)[:2] == (fill.word, fill.word)
    fill.check("switch")


# ---- the one-GPU graph stage ----------------------------------------------------------------------------------------------
GRAPH_EVERY, GRAPH_PARTS = 4, 4                                     # every fourth of the 160 cases, 40 in all, ten a test


@pytest.mark.parametrize("part", range(GRAPH_PARTS))
def test_graph_stage_small_graphs(fill, part):
    """Every fourth case of test_gpu_graph_small.py's family: the default path and one of its twenty variants, in rotation,
    every stage against the oracle (compare_all with the graph) and the variant's markers; every eighth case on a shipped
    handle too."""
    cases = small_graph_cases()[::GRAPH_EVERY]
    per = len(cases) // GRAPH_PARTS
    assert len(cases) == 40 and per * GRAPH_PARTS == len(cases)
    for j, (case, fq, k, min_count, flags) in enumerate(cases[part * per:(part + 1) * per], part * per):
        factory = gs._oracle_factory(fq, k, min_count, flags)
        facts, _ = gs._facts(factory)
        what = "case %d under fill 0x%08x" % (case, fill.word)
        gs.check_run(fq, k, min_count, flags, facts, factory, "default", {}, {}, what)
        name, env, kw = gs.VARIANTS[j % len(gs.VARIANTS)]
        gs.check_run(fq, k, min_count, flags, facts, factory, name, env, kw, what)
        if case % 8 == 0:
            env, kw = gs.VARIANT["shipped"]
            gs.check_run(fq, k, min_count, flags, facts, factory, "shipped", env, kw, what)
    fill.check("graph stage, small graphs, part %d" % part)


WIDE_PICKS = (11, 3, 21, 9, 7, 15)                                  # one case with solid k-mers per key width of the wide family


def test_graph_stage_wide_keys(fill):
    """One case per key width of test_gpu_graph_small.py's wide family (k = 63, 95, 127, 129, 191, 255: two to eight words),
    default path, device writer and a shipped handle."""
    cases = {cs[0]: cs for block in range(WIDE_BLOCKS) for cs in wide_graph_cases(block)}
    words = lambda k: (2 * k + 63) // 64                            # noqa: E731
    assert {words(cases[c][2]) for c in WIDE_PICKS} == {words(cs[2]) for cs in cases.values()}       # every width the family has
    for c in WIDE_PICKS:
        case, fq, k, min_count, flags = cases[c]
        factory = gs._oracle_factory(fq, k, min_count, flags)
        facts, _ = gs._facts(factory)
        assert facts.n_solid > 0, c
        what = "wide case %d under fill 0x%08x" % (case, fill.word)
        gs.check_run(fq, k, min_count, flags, facts, factory, "default", {}, {}, what)
        for name in ("device_writer", "shipped"):
            env, kw = gs.VARIANT[name]
            gs.check_run(fq, k, min_count, flags, facts, factory, name, env, kw, what)
    fill.check("graph stage, wide keys")


# ---- counting -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def counting_reference(k):
    """the input of test_gpu_lowcomplexity.py's counting test and the oracle's answer, once per session"""
    fq = lc.counting_input(k)
    o = run_oracle([fq], k=k, min_count=0, min_qual=0)
    ok_, oc_ = o.distinct()
    return fq, ok_, oc_, o.histo(), o.total_instances


@pytest.mark.parametrize("k", lc.COUNT_KS)
def test_counting(fill, k):
    """The composed low-complexity input of every k of COUNT_KS (one to eight key words) through the default counting mode; at
    k = 31 and 51 through every mode test_gpu_lowcomplexity.py selects.  Distinct table, histogram and instance total are the
    oracle's."""
    fq, ok_, oc_, histo, total = counting_reference(k)
    base = {name: None for name in lc.COUNT_KNOBS}
    envs = lc.counting_envs(fq) if k in (31, 51) else [{}]
    assert envs[0] == {}
    for env in envs:
        lc.count_and_compare(fq, k, dict(base, **env), ok_, oc_, histo, total)
    fill.check("counting k=%d, %d modes" % (k, len(envs)))


# ---- the caller's buffers ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def callers_reads(rest):
    """reads with n_bases % 16 == rest: 400 reads of 100 bases, and one more read of 32 + rest bases"""
    g = synth.random_genome(2000, 611)
    codes, quals = synth.sample_reads(g, 400, 100, 612)
    fq = synth.to_fastq(codes, quals)
    if rest:
        n = 32 + rest
        fq += b"@x\n" + "".join("ACGT"[c] for c in g[100:100 + n]).encode() + b"\n+\n" + b"I" * n + b"\n"
    return fq


@pytest.mark.parametrize("rest", [0, 1, 15])
def test_callers_buffers_of_exactly_the_size_of_the_contract(fill, rest):
    """shk_preprocess_packed_device with d_bases of exactly ceil(n_bases / 16) + 1 words and d_seg_off of exactly n_seg + 1,
    the contract of include/shk.h, both carved out of the middle of a larger tensor of which every other word — the one pad
    word of d_bases included — holds the fill word.  n_bases % 16 = 0, 1, 15: no word, one base and fifteen bases in the last
    data word."""
    import torch
    k = 31
    fq = callers_reads(rest)
    bases, seg, n_bases, n_reads = pack_fastq(fq, k, 0)
    assert n_bases % 16 == rest and len(seg) - 1 >= 400
    n_words = -(-n_bases // 16)
    lead = 64                                                       # words in front of either array (256 bytes: the arrays stay aligned as hipMalloc's are)
    seg_at = lead + -(-(n_words + 1 + lead) // 64) * 64
    host = np.full(seg_at + len(seg) + lead, fill.word, dtype=np.uint32)
    host[lead:lead + n_words] = bases[:n_words]                     # (word lead + n_words, the pad word, keeps the fill word)
    host[seg_at:seg_at + len(seg)] = seg
    dev = torch.device("cuda", 0)
    d_all = torch.from_numpy(host.view(np.int32)).to(dev)
    torch.cuda.synchronize()
    h = AssemblyHelper.new(k, True, 2, 0, 0, False, False, False, False)
    try:
        h.preprocess_packed_device(d_all.data_ptr() + 4 * lead, d_all.data_ptr() + 4 * seg_at, len(seg) - 1, n_bases, n_reads)
        h.assemble()
        torch.cuda.synchronize()
        assert np.array_equal(d_all.cpu().numpy().view(np.uint32), host)      # read, not written
        out = compare_all(h, run_oracle([fq], k=k, min_count=2, min_qual=0), check_graph=True)
        assert out["ncontigs"] >= 1
    finally:
        h.free()
    del d_all
    fill.check("caller's buffers, n_bases %% 16 = %d" % rest)


# ---- the device FASTQ parser ------------------------------------------------------------------------------------------------
FASTQ_CASES = fc.cases()
FASTQ_LEFT_OUT = [fc.BIG]             # fastq_cases.big_case(): 4096 * 4096 + 3 records, 134 MB; not part of fastq_cases.cases()


def test_device_fastq_parser(lib, fill):
    """Every text of tests/fastq_cases.py as test_gpu_fastq_pack.py runs it — the batch word for word against the SPEC packer,
    and the route — but for the one entry that file marks as large (FASTQ_LEFT_OUT)."""
    assert not set(FASTQ_LEFT_OUT) & set(FASTQ_CASES) and len(FASTQ_CASES) >= 240
    for name, c in FASTQ_CASES.items():
        want = fc.reference(name)
        rc, got, route = device_pack_fastq(lib, c.f1, c.f2, c.k, c.min_qual)
        if want is None:
            assert rc == SHK_E_PARSE, (name, rc, route)
            continue
        assert rc == 0, (name, rc, route)
        assert route == c.route, (name, "route", route, "expected", c.route)
        if c.route == "host":
            want = host_pack(lib, joined(c), c.k, c.min_qual)
        assert_same_batch(got, want, name)
    fill.check("device FASTQ parser, %d texts" % len(FASTQ_CASES))


# ---- the device FASTA packer and the header search --------------------------------------------------------------------------
FASTA_CASES = fa.cases()


def test_device_fasta_packer(lib, fill):
    """Every text of tests/fasta_cases.py through shk_device_pack_fasta, as test_gpu_fasta_pack.py runs it: word for word
    against the SPEC packer; a regular text must not take the host route."""
    for name, c in FASTA_CASES.items():
        want = fa.reference(name)
        rc, got, route = device_pack_fasta(lib, c.f1, c.f2, c.k)
        if not c.ok:
            assert want is None
            assert rc == SHK_E_PARSE and route.startswith("host: ") and "FASTA" in route, (name, rc, route)
            continue
        assert rc == 0, (name, rc, route)
        assert route == "device", (name, "a regular text went to", route)
        assert_same_batch(got, want, name)
    fill.check("device FASTA packer, %d texts" % len(FASTA_CASES))


def test_fasta_header_search(lib, fill):
    """The first / last record start of every text of the catalogue (and of its second file), from its first byte, from one
    byte behind every one of its first record starts, from its middle and from its end: the device kernel against the host
    twin and against the rule written out here."""
    n_texts = 0
    for name, c in FASTA_CASES.items():
        for t in (c.f1, c.f2):
            if t is None:
                continue
            n_texts += 1
            starts = [i for i in range(len(t)) if t[i] == 62 and (i == 0 or t[i - 1] == 10)]
            for frm in sorted({0, 1, len(t) // 2, max(len(t) - 1, 0), len(t)} | {s + d for s in starts[:2] + starts[-1:] for d in (0, 1)}):
                got = device_first(lib, t, frm)
                assert got == host_first(lib, t, frm) == min((s for s in starts if s >= frm), default=NONE), (name, frm)
            assert device_last(lib, t) == host_last(lib, t) == (starts[-1] if starts else NONE), name
    fill.check("FASTA header search, %d texts" % n_texts)


# ---- the inflaters ----------------------------------------------------------------------------------------------------------
def test_inflater_bgzf_blocks(lib, fill):
    """tests/deflate_catalogue.py as BGZF blocks, as test_gpu_deflate_streams.py runs it: every legal stream a file of its own
    and all of them one file, taken with zlib's bytes; every stream that is not legal between two legal blocks, declined or
    read as the host reader reads it, never an error; the whole file once more through windows of 64 KiB."""
    for name, d, text in ds.legal():
        assert zlib.decompress(d, -15) == text, name
        blocks = [dw.bgzf_block(d, text)] if text else [ds.lead_block(), dw.bgzf_block(d, text)]
        rc, got, why = ds.device_gunzip(lib, dw.bgzf_file(blocks))
        assert rc == 0, (name, rc, why)
        assert got == (text if text else ds.LEAD), (name, len(got), len(text))
    z, want = ds.whole_file()
    for env in (ds.BGZF_ENV, dict(ds.BGZF_ENV, SHK_GUNZIP_DEVICE_WINDOW=65536)):
        rc, got, why = ds.device_gunzip(lib, z, env)
        assert rc == 0, (rc, why)
        assert got == want
    declined = 0
    for name, d, text, ok in dc.catalogue():
        if ok:
            continue
        z = dw.bgzf_file([ds.lead_block(), dw.bgzf_block(d, text), ds.lead_block()])
        rc, got, why = ds.device_gunzip(lib, z)
        assert rc in (0, 1), (name, rc, why)
        if rc == 0:
            assert (0, got) == ds.host_gunzip(lib, z), name
        declined += rc
    assert declined >= 30, declined                                  # (the floor of test_gpu_deflate_streams.py)
    fill.check("inflater, BGZF blocks")


def test_inflater_one_member(lib, fill):
    """The catalogue as ONE gzip member (deflate_catalogue.device_member: every legal entry between landing blocks), cut
    every 4096 bytes: taken, zlib's bytes.  And the refusals the catalogue states, each with its own reason: a bad first
    block, distance symbol 30 in a later chunk, a match that reaches in front of the stream from a later chunk, runs of 258 at
    distance 1 that outgrow their room (taken once the room is given)."""
    env = dict(ds.MEMBER_ENV, SHK_GUNZIP_DEVICE_CHUNK=4096)
    z, text, _ = ds.odd_member()
    rc, got, why = ds.device_gunzip(lib, z, env)
    assert rc == 0, (rc, why)
    assert got == text
    for refuse, reason in (("first", "a chunk does not end where the next begins"), ("symbol 30", "a chunk does not end where the next begins"),
                           ("front", "a back-reference in front of the stream")):
        d, t, _m = dc.device_member(150000, refuse)
        with pytest.raises(zlib.error):
            zlib.decompress(d, -15)
        rc, got, why = ds.device_gunzip(lib, dw.gzip_member(d, t), env)
        assert (rc, why) == (1, reason), refuse
    d, t, _ = dc.runs_member(150000, 80)
    assert zlib.decompress(d, -15) == t
    z = dw.gzip_member(d, t)
    rc, got, why = ds.device_gunzip(lib, z, env)
    assert (rc, why) == (1, "a chunk inflates beyond its room")
    rc, got, why = ds.device_gunzip(lib, z, dict(env, SHK_GUNZIP_DEVICE_RATIO=2 * -(-len(t) // len(d))))
    assert rc == 0, (rc, why)
    assert got == t
    fill.check("inflater, one member")


# ---- the BGZF writer --------------------------------------------------------------------------------------------------------
def json_escaped(text):
    """text as JSON string content with the four escapes the writer makes, or None where it holds a byte that would need another"""
    if any(b >= 0x7F or (b < 0x20 and b not in (9, 10)) for b in text):
        return None
    return text.replace(b"\\", b"\\\\").replace(b'"', b'\\"').replace(b"\n", b"\\n").replace(b"\t", b"\\t")


def test_bgzf_writer(lib, fill):
    """tests/bgzf_write_cases.py through shk_device_bgzf_compress: the host encoder's file byte for byte, a well-formed BGZF
    file of the text (check_file), the golden outputs of tests/golden/bgzf_write_outputs.json among the texts.  Through
    shk_device_bgzf_compress_escaped: every text that JSON string content can spell with \\n \\t \\" \\\\, the same file."""
    golden = bw.golden_outputs()
    escaped = 0
    for name, text in bw.catalogue():
        data = bgz.device_file(lib, text)
        assert not isinstance(data, int), (name, data)
        assert data == host_file(lib, text), name
        bw.check_file(data, text)
        assert gzip.decompress(data) == text, name
        if name.startswith("golden_"):
            assert text == golden[name[len("golden_"):]].encode()
        esc = json_escaped(text)
        if esc is not None:
            assert json.loads(b'"' + esc + b'"').encode() == text, name
            assert bgz.device_file(lib, esc, escaped=True) == data, name
            escaped += 1
    assert escaped >= 9, escaped                                     # empty, one_byte, the three acgt, the four golden
    fill.check("BGZF writer")


# ---- the text writer and the unitig level -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def writer_reference(k, err):
    """the input of test_gpu_text_writer.test_device_text_writer_equals_the_oracle_writer for this k: the oracle's unitigs on a
    random strand in a random order, and the oracle's JSON"""
    g, fq = make_dataset(30000, 14, read_len=150 if k < 128 else 400, err=err, seed=900 + k)
    o = run_oracle([fq], k=k, min_count=1, min_qual=0, no_bubble_collapse=True, no_dead_end_removal=True)
    o.assemble()
    cs, kcs = o.contigs(), o.contig_kc()
    rng = np.random.default_rng(k)
    items = tuple((revcomp(cs[i]) if rng.integers(0, 2) else cs[i], kcs[i]) for i in rng.permutation(len(cs)))
    return items, o.assembly_json()


@pytest.mark.parametrize("k,err", [(31, 0.01), (161, 0.004), (255, 0.003)])
def test_text_writer_against_the_oracle(lib, fill, k, err):
    items, want = writer_reference(k, err)
    assert len(items) > 20
    host, dev = tw._both(lib, list(items), k)
    assert dev == want and host == want
    fill.check("text writer k=%d, %d contigs" % (k, len(items)))


def test_text_writer_hand_made_texts(lib, fill):
    """the hand-made texts of test_gpu_text_writer.py (k = 15 and 31), as given and with every contig turned; no contig at all"""
    assert {k for _, k in tw._HAND.values()} == {15, 31}
    for name, (contigs, k) in sorted(tw._HAND.items()):
        for flip in (False, True):
            items = [(revcomp(s) if flip else s, c) for s, c in contigs]
            host, dev = tw._both(lib, items, k)
            assert dev == host, (name, flip)
    seqs, off, kc = tw._arrays([])
    dev, why = tw._device_raw(lib, seqs, off, kc, 0, 31)
    assert dev == tw.EMPTY == tw._host_raw(lib, seqs, off, kc, 0, 31), why
    fill.check("text writer, hand-made texts")


def test_unitig_chains(fill):
    """shk_device_unitig_chains against the host walk: the first 40 random cases of tests/unitig_chains_cases.py (ten at each
    k of KS = 31, 63, 127, 255) and, at each k, chains and rings around the widths of a wave and a workgroup."""
    for i in range(40):
        chains_device_equals_host(random_case(i))
    for k in KS:
        B = Builder(k, 70 + k)
        B.chain_pair(1); B.chain_pair(65); B.self_chain(257); B.ring_pair(64); B.self_ring(3); B.circ_record(); B.dead_pair()
        chains_device_equals_host(B.build())
    assert chains_device_equals_host(Builder(31, 1).build()) == "need_min :\n"
    fill.check("unitig chains")


# ---- further entry points, as their own tests run them ----------------------------------------------------------------------
def test_further_entry_points(lib, fill):
    """Beyond the catalogues above: whole tests of three more entry points, called as they stand (as test_gpu_unitig_chains.py
    calls those of test_gpu_unitig_graph.py), each with its own reference — shk_device_first_record_start against the host
    rule; shk_device_unitig_assemble on three hand-built graphs against the host text; shk_get_assembly_bgzf and
    shk_request_assembly_bgzf on the four small assemblies, whose files must inflate (gzip) to the fields of the JSON."""
    sq.test_device_first_record_start_equals_the_host_function(lib)
    ug.case_three_tips(31, "any")
    ug.case_bubble_at_the_limit(63, "hi")
    ug.test_a_ring_of_several_records_that_forms_after_a_removal()
    for name in bgz.ASSEMBLIES:
        bgz.test_assembly_files_inflate_to_the_fields(lib, name)
    fill.check("further entry points")


# ---- sharded, one rank, in this process -------------------------------------------------------------------------------------
def test_sharded_one_rank(fill):
    """Every eighth small-graph case through shk_shard_preprocess and the collective shk_assemble on a one-rank communicator
    (made under the fill: its stage buffer is filled too), default path and one variant of test_gpu_shard_graph_small.py in
    rotation: both texts are the oracle's."""
    from sparrowhawk_amd.dist import LibComm
    tally, runs = {}, {}
    comm = LibComm(0, 1)
    try:
        for j, c in enumerate(range(0, sgs.SMALL_GRAPH_CASES, 8)):
            sgs.check_one_rank(comm, "small", c, [sgs.DEFAULT, sgs.VARIANTS[j % len(sgs.VARIANTS)]], tally, runs)
    finally:
        comm.free()
    assert runs["default"] == 20 and sum(runs.values()) == 40, runs
    fill.check("sharded, one rank")


# ---- sharded, three ranks -----------------------------------------------------------------------------------------------------
RANKS_PICKS = [(16, "default"), (32, "seg_cap1"), (48, "unitig_device"), (120, "all_device"), (152, "shipped_all_device")]
RANKS_PORT = 29897


def test_sharded_three_ranks():
    """ONE launch of tests/dist_worker.py rccl_many on 3 ranks (not a power of two) sharing the GPU, their bytes through
    tests/mock_rccl at its most hostile: five small-graph cases, each with a variant of test_gpu_shard_graph_small.py, and the
    genome of k + 5 bases of test_dist.py that leaves a rank without a solid k-mer — every case under each of the three
    words (the worker's "pool_fill" key sets the word before the handle is made).  The ranks start with SHK_POOL_FILL in
    their environment, so the communicator's stage buffer is filled as well.  Every rank returns the oracle's bytes."""
    world = 3
    variants = {name: (env, kw) for name, env, kw in sgs.ALL}
    six = []
    for c, name in RANKS_PICKS:
        case, fq, k, min_count, flags = sgs.the_case("small", c)
        env, kw = variants[name]
        shipped = bool(kw.get("shipped"))
        f = sgs.facts_of("small", c)
        six.append(("case %d %s" % (c, name), fq, dict(k=k, min_count=min_count, min_qual=0, verbose=not shipped, env=sgs.run_env(env, shipped), **flags),
                    (f.pre, f.asm), f.nkmers))
    tiny = synth.random_genome(46, 8470 + world)
    codes, quals = synth.sample_reads(tiny, 12, 46, 8471 + world, err=0.0, circular=False)
    fq, pr = synth.to_fastq(codes, quals), dict(k=41, min_count=2, min_qual=0)
    pre, asm = _oracle_jsons(fq, pr)
    six.append(("a genome of k + 5 bases", fq, dict(pr, env=sgs.run_env({}, False)), (pre, asm), json.loads(pre)["nkmers"]))
    assert len(six) == 6 and six[-1][4] > 0
    runs = [(what, fq, dict(params, pool_fill="%08x" % word), ref, nk, word) for word in WORDS for what, fq, params, ref, nk in six]
    env_was = {name: os.environ.get(name) for name in ("SHK_RCCL_LIBRARY", "MOCK_RCCL_JITTER", "SHK_POOL_FILL")}
    os.environ.update(SHK_RCCL_LIBRARY=mock_rccl_library(), MOCK_RCCL_JITTER="1", SHK_POOL_FILL="00000001")
    try:
        with tempfile.TemporaryDirectory() as d:
            cfgp = _write_cases(d, [(fq, params) for _, fq, params, _, _, _ in runs])
            out = os.path.join(d, "res")
            launch(world, ["rccl_many", out, cfgp], RANKS_PORT, timeout=420 + 3 * len(runs))
            res = [json.load(open(f"{out}.{r}")) for r in range(world)]
    finally:
        for name, v in env_was.items():
            if v is None:
                os.environ.pop(name, None)
            else:
                os.environ[name] = v
    assert all(len(res[r]) == len(runs) for r in range(world))
    for i, (what, fq, params, (pre, asm), nkmers, word) in enumerate(runs):
        msg = "%s under fill 0x%08x on %d ranks" % (what, word, world)
        for r in range(world):
            assert "error" not in res[r][i], (msg, r, res[r][i])
            assert res[r][i]["pool_filled_bytes"] > 0, msg + f": rank {r} ran unfilled"
            assert res[r][i]["pre"] == pre, msg + f": preprocessing info differs on rank {r}"
            assert res[r][i]["asm"] == asm, msg + f": assembly differs on rank {r}"
        rows = [res[r][i]["n_solid_local"] for r in range(world)]
        assert sum(rows) == nkmers, (msg, rows)
        if what.startswith("a genome"):
            assert min(rows) == 0, (msg, rows)                      # a rank without a single solid k-mer
    print("pool fill, three ranks: bytes filled per rank and run", [[res[r][i]["pool_filled_bytes"] for r in range(world)] for i in range(len(runs))])
