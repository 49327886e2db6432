"""The texts the BGZF writer (SPEC S11a; csrc/deflate_write.h, csrc/bgzf_write_gpu.hip) is tested on, shared by the CPU tests
(test_bgzf_write_host.py) and the GPU tests (test_gpu_bgzf_write.py), and the reader that takes a file apart block by block.
Every text is at most a few blocks of 65 280 bytes."""
import functools
import json
import os
import struct
import zlib

import numpy as np

BLOCK = 65280                       # bytes of text per block (bgzip's own figure)
EOF_MARKER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")     # bgzip's empty last block
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bgzf_write_outputs.json")
FIELDS = ("outfasta", "outdot", "outgfa", "outgfav2")


def acgt_lines(n, seed, width=60):
    """n bytes of seeded ACGT in lines of `width` bases"""
    rng = np.random.default_rng(seed)
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)]
    bases[width::width + 1] = 10
    return bases.tobytes()


def fibonacci_counts():
    """22 counts 1, 1, 2, 3, 5 ... F22: 46 367 in all.  Huffman's tree over them is a comb 21 deep where ties go the other way;
    with end-of-block as a third 1 and the library's tie rule it is 12 deep (test_bgzf_write_host.py says why)."""
    f = [1, 1]
    while len(f) < 22:
        f.append(f[-1] + f[-2])
    return f


def lucas_counts():
    """1, 1, 3, 4, 7, 11 ... 24476 (22 counts, 64 077 in all): behind end-of-block and the two ones, every count is above the
    weight of everything in front of it joined, so Huffman's tree is a comb 22 deep whatever the tie rule.  The text that
    needs the length limiter under the library's rule too."""
    c = [1, 1, 3, 4]
    while len(c) < 22:
        c.append(c[-1] + c[-2])
    return c


def fibonacci_text(seed=5, counts=None):
    counts = counts or fibonacci_counts()
    t = np.concatenate([np.full(c, 40 + i, dtype=np.uint8) for i, c in enumerate(counts)])
    np.random.default_rng(seed).shuffle(t)
    return t.tobytes()


@functools.lru_cache(maxsize=None)
def golden_outputs():
    """the four outputs of a small assembly with links, as the host writer wrote them (tests/golden/bgzf_write_outputs.json)"""
    with open(GOLDEN) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def catalogue():
    """[(name, text)]"""
    rng = np.random.default_rng(77)
    g = golden_outputs()
    cases = [("empty", b""), ("one_byte", b"A")]
    cases += [("acgt_%d" % n, acgt_lines(n, 100 + i)) for i, n in enumerate((BLOCK - 1, BLOCK, BLOCK + 1))]
    cases.append(("one_value", b"G" * BLOCK))
    cases.append(("all_values_equal", np.random.default_rng(3).permutation(np.repeat(np.arange(256, dtype=np.uint8), 255)).tobytes()))
    cases.append(("random_bytes", rng.integers(0, 256, BLOCK + 4000, dtype=np.uint8).tobytes()))
    cases.append(("fibonacci", fibonacci_text()))
    cases.append(("lucas", fibonacci_text(6, lucas_counts())))
    cases += [("golden_" + name, g[name].encode()) for name in FIELDS]
    # a Huffman block, a stored one and a short Huffman one: more than 65 536 bytes of file, so the device inflater takes it
    # with SHK_GUNZIP_DEVICE_MIN=65536
    cases.append(("three_blocks", acgt_lines(BLOCK, 9) + rng.integers(0, 256, BLOCK, dtype=np.uint8).tobytes() + g["outgfa"].encode() * 3))
    return cases


STORED_CASES = ("random_bytes",)     # every block of these must come out stored (BTYPE = 0)


def histogram(block_text):
    """the 257 counts of a block: its bytes and end-of-block"""
    c = np.bincount(np.frombuffer(block_text, dtype=np.uint8), minlength=256).astype(np.uint32)
    return np.concatenate([c, np.ones(1, dtype=np.uint32)])


def parse_bgzf(data):
    """[{bsize, deflate, crc, isize, btype}] of a BGZF chain that must cover `data` exactly (asserts the framing)"""
    blocks, at = [], 0
    while at < len(data):
        assert len(data) - at >= 28, "a tail too short for a block"
        head = data[at:at + 18]
        assert head[:4] == b"\x1f\x8b\x08\x04" and head[10:12] == b"\x06\x00", "not a gzip member with one extra field of 6 bytes"
        assert head[12:16] == b"BC\x02\x00", "no BC subfield"
        bsize = struct.unpack("<H", head[16:18])[0] + 1
        assert at + bsize <= len(data), "BSIZE runs past the file"
        deflate = data[at + 18:at + bsize - 8]
        crc, isize = struct.unpack("<II", data[at + bsize - 8:at + bsize])
        blocks.append(dict(bsize=bsize, deflate=deflate, crc=crc, isize=isize, btype=(deflate[0] >> 1) & 3, bfinal=deflate[0] & 1))
        at += bsize
    return blocks


def check_file(data, text):
    """everything SPEC S11a says of the file of `text`; returns the blocks in front of the end marker"""
    import gzip
    assert data[-28:] == EOF_MARKER
    assert gzip.decompress(data) == text
    blocks = parse_bgzf(data)
    assert len(blocks) == (len(text) + BLOCK - 1) // BLOCK + 1
    at = 0
    for i, b in enumerate(blocks[:-1]):
        want = text[at:at + BLOCK]
        assert b["isize"] == len(want) and 0 < b["isize"] <= BLOCK, (i, b["isize"])
        assert b["crc"] == zlib.crc32(want), i
        assert b["bfinal"] == 1 and b["btype"] in (0, 2), (i, b["btype"])
        assert zlib.decompress(b["deflate"], -15) == want, i                 # the block alone, as a raw deflate stream that ends in it
        if b["btype"] == 0:
            assert len(b["deflate"]) == 5 + len(want)
        else:
            assert len(b["deflate"]) < 5 + len(want), "a Huffman block that is not strictly smaller than the stored form"
        at += len(want)
    assert at == len(text) and blocks[-1]["isize"] == 0
    return blocks[:-1]
