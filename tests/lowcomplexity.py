"""The low-complexity family: reads as real isolates have them and i.i.d. uniform sequence never does — genomes of 8 to 92 %
A+T, homopolymer runs, microsatellites (units that equal their own reverse complement among them), interrupted repeats,
read tails and whole reads of poly-G.  Every other input of the suite, of the fuzzers and of the benchmark draws its bases
uniformly; its "repeats" are copies of random sequence.

What such sequence asks of the product that uniform sequence does not:
  - every k-mer of a stretch of period <= 8 has the same minimiser (a k-mer window holds >= 8 m-mers at every k, so every window
    holds the same set of m-mers): pass 1 cuts such a run at the record cap alone (count_part.h, k_partition), at any P;
  - a k-mer occurs several times in one record, with its reverse complement, and the record may be its own reverse
    complement ((AT)n, (ACGT)n, (AATT)n: the no-decision branch of rec_canonicalise);
  - many lanes of a wave hold the same record or the same key at the same time (rec_insert, lds_insert);
  - a whole repeat lands in one minimiser partition, and one key has more instances than a bucket region can be given;
  - the graph has self-loops next to real exits, nodes whose out-neighbour is their own mirror, rings of 2 ... 8 nodes (none
    has a sampled node: k_orphan_cycles), isolated nodes linked to themselves, chains closed onto their own mirror strand by a hairpin link at either end, tips
    and bubbles whose walks pass a self-loop.  (What the campaign's cases reach of
    this is counted, with floors, by test_lowcomplexity.test_low_complexity_campaign_reaches_every_class.)

low_complexity_case has the signature and the flag rules of test_oracle._random_graph_case.  The class predicates at the end
are pure Python on the reads: they say what an input reaches, and never look at what the product made of it."""
import os

import numpy as np

from util import parse_fastq, revcomp

# repeat units; A/T, C/G, AT, CG, TA, GC, ACGT, AATT, AGCT, ACGCGT and AACCGGTT equal their own reverse complement
UNITS = ["A", "C", "G", "T", "AT", "CG", "AC", "AG", "TA", "GC", "AAT", "ACG", "CCG", "ACGT", "AATT", "AGCT", "AAAT", "AACCT",
         "ACGCGT", "AAAAAC", "ACACAG", "AACCGGTT"]
K_NARROW = [15, 17, 21, 25, 31, 33, 41]
K_WIDE = [63, 65, 95, 127, 129, 191, 255]
MAX_PERIOD = 8                                             # the shortest minimiser window of pass 1 (pipeline.hip, part_win)


def composition(at):
    """base probabilities (A, C, G, T) of a genome whose A+T share is `at`"""
    return [at / 2, (1 - at) / 2, (1 - at) / 2, at / 2]


def repeat_of(unit, n, phase):
    """n bases of (unit)* starting `phase` bases into the unit"""
    return (unit * (n // len(unit) + 2))[phase:][:n]


def substitute(base, step):
    return "ACGT"[("ACGT".index(base) + step) % 4]


def low_complexity_case(rng, case, wide=False):
    """One input of the family: (fastq bytes, k, min_count, flags).  style = case % 6 — 0: composition alone (8 or 92 % A+T);
    1, 2: one to three inserts of a unit of UNITS; 3: the same with one substitution inside the repeat (an interrupted
    microsatellite); 4: the same, and a fifth of the reads get a poly-G tail from a random position (position 0: a whole poly-G
    read); 5: half of the units are random, 2 ... k - 1 bases long.
    wide: keys of two to eight words, the backbone 4 k longer, reads k + 120 long, and inserts of k + 64 and k + 100 bases
    as well, so that a stretch of period <= 8 inside one read exceeds k - 1 + max_n bases; off, no draw changes."""
    k = int(rng.choice(K_WIDE if wide else K_NARROW))
    L = int(rng.integers(300, 1501)) + (4 * k if wide else 0)
    style = case % 6
    at = float(rng.choice([0.5, 0.1, 0.9])) if style != 0 else float(rng.choice([0.08, 0.92]))
    g = "".join(rng.choice(list("ACGT"), L, p=composition(at)))
    lengths = [k - 2, k, k + 1, 2 * k, 70, 200] + ([k + 64, k + 100] if wide else [])
    for _ in range(int(rng.integers(1, 4)) if style else 0):
        u = UNITS[int(rng.integers(0, len(UNITS)))]
        if style == 5 and rng.random() < 0.5:
            u = "".join(rng.choice(list("ACGT"), int(rng.integers(2, k))))
        n = int(rng.choice(lengths))
        rep = repeat_of(u, n, int(rng.integers(0, len(u))))
        if style == 3:
            q = int(rng.integers(1, n - 1))
            rep = rep[:q] + substitute(rep[q], 1) + rep[q + 1:]
        pos = int(rng.integers(0, len(g)))
        g = g[:pos] + rep + g[pos:]
    cov = float(rng.choice([6, 16, 30]))
    err = float(rng.choice([0.0, 0.003, 0.01]))
    rl = k + 120 if wide else int(rng.choice([60, 100, 150]))
    recs = []
    for _ in range(max(2, int(len(g) * cov / rl))):
        ll = min(rl, len(g))
        s0 = int(rng.integers(0, len(g) - ll + 1))
        rd = list(g[s0:s0 + ll])
        for j in range(len(rd)):
            if rng.random() < err:
                rd[j] = substitute(rd[j], int(rng.integers(1, 4)))
        if style == 4 and rng.random() < 0.2:
            c = int(rng.integers(0, len(rd)))
            rd[c:] = "G" * (len(rd) - c)
        rd = "".join(rd)
        if rng.random() < 0.5:
            rd = revcomp(rd)
        recs.append(f"@r{len(recs)}\n{rd}\n+\n{'I' * len(rd)}\n")
    min_count = int(rng.choice([0, 1, 1, 2, 3]))
    if case % 3 == 0:
        # satellites: one or two components that are nothing but a repeat — reads spelled from a unit alone, without errors,
        # often enough to stay solid at every min_count.  A unit of primitive period p that is not an inserted unit of the
        # backbone is a ring of p nodes on its own (poly-G: one node linked to itself, which is no ring); a unit that equals a rotation of its reverse complement
        # (AT, CG, ACGT, AATT, AGCT, ACGCGT, AACCGGTT) folds into a chain of p / 2 nodes closed by a hairpin link at either end.
        for _ in range(int(rng.integers(1, 3))):
            u = UNITS[int(rng.integers(0, len(UNITS)))]
            for _ in range(int(rng.integers(4, 8))):
                rd = repeat_of(u, rl, int(rng.integers(0, len(u))))
                if rng.random() < 0.5:
                    rd = revcomp(rd)
                recs.insert(int(rng.integers(0, len(recs) + 1)), f"@s{len(recs)}\n{rd}\n+\n{'I' * len(rd)}\n")
    flags = dict(no_bubble_collapse=bool(case % 7 == 3), no_dead_end_removal=bool(case % 11 == 5))
    return "".join(recs).encode(), k, min_count, flags


NARROW_CASES, WIDE_CASES = 120, 12
_cache = {}


def _cases(name, default_seed, upto, wide):
    seed = int(os.environ.get(name, default_seed))
    rng, got = _cache.setdefault((name, seed), (np.random.default_rng(seed), []))
    while len(got) < upto:                                 # (drawn once per session, in order)
        got.append((len(got),) + low_complexity_case(rng, len(got), wide=wide))
    return got[:upto]


def narrow_cases(upto=NARROW_CASES):
    """Cases 0 ... upto-1 of the campaign (seed SHK_LOW_COMPLEXITY_SEED), always drawn from case 0 of one generator, so that a
    case number names the same input whichever test asks for it: (case, fastq, k, min_count, flags)."""
    return _cases("SHK_LOW_COMPLEXITY_SEED", 1, upto, False)


def wide_cases(upto=WIDE_CASES):
    """The same at k = 63 ... 255 (seed SHK_LOW_COMPLEXITY_WIDE_SEED)."""
    return _cases("SHK_LOW_COMPLEXITY_WIDE_SEED", 2, upto, True)


# ---- a genome and reads with the family's features, as arrays (the counting test's input, the fuzzer's genomes) -------------
_ASCII_TO_CODE = np.zeros(256, dtype=np.uint8)
for _i, _c in enumerate("ACGT"):
    _ASCII_TO_CODE[ord(_c)] = _i


def str_to_codes(s):
    return _ASCII_TO_CODE[np.frombuffer(s.encode(), dtype=np.uint8)]


def skewed_genome(rng, n, at):
    """n base codes (0 ... 3 = ACGT) with an A+T share of `at`"""
    return rng.choice(4, n, p=composition(at)).astype(np.uint8)


def with_inserts(rng, g, inserts):
    """the genome (base codes) with every (unit, bases) of `inserts` put in at a random place and a random phase"""
    for unit, n in inserts:
        rep = str_to_codes(repeat_of(unit, n, int(rng.integers(0, len(unit)))))
        pos = int(rng.integers(0, len(g) + 1))
        g = np.concatenate([g[:pos], rep, g[pos:]])
    return g


def low_complexity_genome(rng, n, k):
    """A genome of about n bases for the long fuzzing campaigns: the family's compositions and one to three inserts."""
    g = skewed_genome(rng, n, float(rng.choice([0.08, 0.1, 0.5, 0.9, 0.92])))
    inserts = [(UNITS[int(rng.integers(0, len(UNITS)))], int(rng.choice([k - 2, k, k + 1, 2 * k, 70, 200, k + 64, k + 100])))
               for _ in range(int(rng.integers(1, 4)))]
    return with_inserts(rng, g, inserts)


def composed_counting_input(k, seed):
    """The counting test's input at one k: a 20 kbp backbone, half of it at 15 % G+C, one insert of EVERY unit at 200 and at
    k + 100 bases, 25-fold coverage by reads max(150, k + 120) long with 0.5 % substitutions, a tenth of the reads with a
    poly-G tail from a random position, each read reverse-complemented with probability 1/2.  FASTQ bytes, quality 'I'."""
    rng = np.random.default_rng(seed)
    g = np.concatenate([skewed_genome(rng, 10000, 0.85), skewed_genome(rng, 10000, 0.5)])
    g = with_inserts(rng, g, [(u, n) for u in UNITS for n in (200, k + 100)])
    rl = max(150, k + 120)
    n_reads = len(g) * 25 // rl
    starts = rng.integers(0, len(g) - rl + 1, n_reads)
    reads = g[starts[:, None] + np.arange(rl)[None, :]]
    hit = rng.random(reads.shape) < 0.005
    reads = np.where(hit, (reads + rng.integers(1, 4, reads.shape)) % 4, reads).astype(np.uint8)
    tail = np.where(rng.random(n_reads) < 0.1, rng.integers(0, rl, n_reads), rl)
    reads[np.arange(rl)[None, :] >= tail[:, None]] = 2
    flip = rng.random(n_reads) < 0.5
    reads[flip] = (3 - reads[flip])[:, ::-1]
    text = np.frombuffer(b"ACGT", dtype=np.uint8)[reads]
    qual = "I" * rl
    return "".join(f"@r{i}\n{text[i].tobytes().decode()}\n+\n{qual}\n" for i in range(n_reads)).encode()


# ---- class predicates: pure Python on the reads ---------------------------------------------------------------------------
def record_cap_of(k):
    """k-mers a pass-1 record holds at most: pipeline.hip, count_batch_impl — pp_.max_n = min(32 RW - 3 - (k - 1), 63) with
    RW = 2 W words per record, W = ceil(2 k / 64)."""
    W = (2 * k + 63) // 64
    return min(64 * W - 3 - (k - 1), 63)


def longest_periodic_stretch(read, max_period=MAX_PERIOD):
    """the longest stretch of the read with a period of 1 ... max_period bases (a stretch of period p has >= p bases)"""
    a = np.frombuffer(read.encode(), dtype=np.uint8)
    best = 0
    for p in range(1, max_period + 1):
        if len(a) <= p:
            break
        differs = np.flatnonzero(a[p:] != a[:-p])
        edges = np.concatenate([[-1], differs, [len(a) - p]])
        run = int(np.max(np.diff(edges))) - 1              # positions i in a row with a[i + p] == a[i]
        if run > 0:
            best = max(best, run + p)
    return best


def canonical_counts(fq, k):
    """canonical k-mer (as a string) -> count, over reads whose every base is ACGT at a quality nothing masks"""
    counts = {}
    for rd, _q in parse_fastq(fq):
        for i in range(len(rd) - k + 1):
            s = rd[i:i + k]
            r = revcomp(s)
            x = s if s < r else r
            counts[x] = counts.get(x, 0) + 1
    return counts


def classes(fq, k, counts=None):
    """Which of the family's classes the reads reach:
    homopolymer           some canonical k-mer is one base repeated (a node with a self-loop);
    own_mirror_neighbour  some k-mer x has revcomp(x) among x[1:] + b (a hairpin link, not simple under SPEC S10);
    record_cap            some read holds a stretch of period <= 8 of at least k + max_n bases: more than max_n k-mers in a row
                          with one minimiser, so pass 1 cuts the run at the record cap;
    heavy                 the largest k-mer count is >= 20 x the median count."""
    if counts is None:
        counts = canonical_counts(fq, k)
    if not counts:
        return dict(homopolymer=False, own_mirror_neighbour=False, record_cap=False, heavy=False)
    stretch = max(longest_periodic_stretch(rd) for rd, _q in parse_fastq(fq))
    values = sorted(counts.values())
    return dict(homopolymer=any(x == x[0] * k for x in counts),
                own_mirror_neighbour=any(revcomp(x) in (x[1:] + b for b in "ACGT") or x in (revcomp(x)[1:] + b for b in "ACGT")
                                         for x in counts),
                record_cap=stretch >= k + record_cap_of(k),
                heavy=values[-1] >= 20 * values[len(values) // 2])


def rings_of(contigs, gfa1, k):
    """The circular unitigs of an assembly, from the oracle's contigs and GFA1 text: a contig with a link to itself on one
    strand, NO other link and at least two nodes.  (The self-link alone does not make a ring: a homopolymer node with real exits is a one-node
    contig with such a link and others.  Every link around a circular unitig is simple, so it has none but its own.)
    Returns the node count of each.  No ring is its own mirror strand while k is odd: v -> rc(v) maps such a ring onto itself
    against its direction, so it fixes a node (v = rc(v): impossible at odd k) or a link v -> rc(v) (a hairpin link, which is
    not simple, SPEC S10).  A repeat whose unit equals its reverse complement folds into a chain closed by two hairpin links
    instead: hairpin_closed_of."""
    self_linked, others = set(), set()
    for l in gfa1.split("\n"):
        if l.startswith("L\t"):
            f = l.split("\t")
            if f[1] == f[3] and f[2] == f[4]:
                self_linked.add(int(f[1]))
            else:
                others.update((int(f[1]), int(f[3])))
    nodes = [len(contigs[i - 1]) - (k - 1) for i in sorted(self_linked - others)]
    return [n for n in nodes if n >= 2]


def isolated_self_loops_of(contigs, gfa1, k):
    """One-node contigs whose only link is onto themselves: an isolated homopolymer component.  Not a ring — v -> v is not a
    simple link (SPEC S10), so the node is a linear chain of one with a link to itself.  Returns how many."""
    self_linked, others = set(), set()
    for l in gfa1.split("\n"):
        if l.startswith("L\t"):
            f = l.split("\t")
            (self_linked.add(int(f[1])) if f[1] == f[3] and f[2] == f[4] else others.update((int(f[1]), int(f[3]))))
    return sum(1 for i in self_linked - others if len(contigs[i - 1]) == k)


def hairpin_closed_of(gfa1):
    """Contigs whose only links are the two hairpin links onto their own other strand (i + -> i - and i - -> i +): what an
    isolated repeat of a unit that equals a rotation of its reverse complement folds into — (AT)n one node, (ACGT)n two,
    (ACGCGT)n three, (AACCGGTT)n four.  Returns their numbers."""
    own, others = {}, set()
    for l in gfa1.split("\n"):
        if l.startswith("L\t"):
            f = l.split("\t")
            if f[1] == f[3] and f[2] != f[4]:
                own.setdefault(int(f[1]), set()).add(f[2])
            else:
                others.update((int(f[1]), int(f[3])))
    return sorted(i for i, signs in own.items() if signs == {"+", "-"} and i not in others)
