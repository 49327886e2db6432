"""The DEVICE inflater (csrc/inflate_gpu.hip, through shk_device_gunzip) against Python's zlib on the streams of
tools/fuzz_gunzip.py: members of 70 kB ... 20 MB made with random levels, strategies, windows, flush points and member counts
from FASTQ-like text, runs, binary data and mixtures, each also truncated and with single bits flipped.  The device inflater
either hands back exactly zlib's bytes or declines (the product then reads the member on the host, which owns the error
messages): it must NEVER return other bytes.  Needs a GPU.  Usage: python tools/fuzz_gunzip_device.py [cases] [seed] [bgzf]
bgzf: BGZF (bgzip) files instead — blocks of random sizes (1 ... 65 280 bytes of text) and levels, empty blocks anywhere,
with or without the end-of-file block.  Every intact file must be TAKEN with its text's bytes (this path has no speculative
step); a damaged one (cut short, bits flipped, BSIZE / ISIZE / CRC-32 fields changed) is declined or comes back as the host
reader (shk_host_gunzip) reads it.
bgzf written: the same campaign on files whose blocks come from the bit-level writer of the tests (tests/deflate_writer.py)
instead of zlib's encoder: random token lists (greedy parses with random match limits), stored, fixed and dynamic blocks in
turn, random complete code-length sets with a longest code of 7 ... 15 bits, the header's length list written literally, with
greedy runs or with runs that stop at the literal/distance boundary.  Texts are smaller (the writer is pure Python)."""
import ctypes as C
import os
import sys
import time
import zlib
from collections import Counter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))             # (deflate_writer, for `bgzf written`)
os.environ.setdefault("SHK_GUNZIP_DEVICE_MIN", "32768")
import torch  # noqa: F401  (one HIP runtime)
import fuzz_gunzip as fg

L = fg.L
rng = fg.rng
n_cases = fg.n_cases


def device_gunzip(z):
    out, n, why, ms = C.c_void_p(), C.c_size_t(), C.c_char_p(), C.c_double()
    rc = L.shk_device_gunzip(z, len(z), C.byref(out), C.byref(n), C.byref(why), C.byref(ms))
    if rc == 0:
        got = C.string_at(out.value, n.value) if n.value else b""
        L.shk_host_free(out)
        return 0, got, "", ms.value
    return rc, None, (why.value or b"").decode(), ms.value


def bgzf_file(text):
    """(file, [(offset, BSIZE)]): `text` in blocks of random sizes and levels, empty blocks strewn in"""
    from sparrowhawk_amd import synth
    small = rng.random() < 0.3                               # thousands of tiny blocks at times
    parts, p = [], 0
    while p < len(text):
        n = int(rng.integers(1, 2000)) if small else int(rng.choice([65280, 65280, 30000, int(rng.integers(1, 65281))]))
        parts.append(synth.bgzf_compress(text[p:p + n], block=65280, level=int(rng.integers(0, 10)), eof=False))
        p += n
        if rng.random() < 0.02:
            parts.append(synth.bgzf_compress(b""))
    if rng.random() < 0.7:
        parts.append(synth.bgzf_compress(b""))
    offs, o = [], 0
    for b in parts:
        offs.append((o, len(b))); o += len(b)
    return b"".join(parts), offs


def written_bgzf_file(text):
    """(file, [(offset, BSIZE)]): `text` in BGZF blocks of 1 ... 20 000 bytes, each a stream of one to four blocks written bit by bit"""
    import deflate_writer as dw

    def noisy_lengths(freqs):
        f = [x * float(rng.integers(1, 50)) if x else 0 for x in freqs]
        n = sum(1 for x in f if x)
        if n < 2:
            return dw.huffman_lengths(f, 15)
        m = int(rng.integers(7, 16))
        if m + 1 <= n <= m + (1 << (m - 1)) and rng.random() < 0.5:
            return dw.lengths_with_max(f, m)
        return dw.huffman_lengths(f, max(m, n.bit_length()))
    parts, p = [], 0
    while p < len(text):
        n = int(rng.choice([int(rng.integers(1, 40)), int(rng.integers(1, 3000)), int(rng.integers(1, 20000))]))
        piece, s, q = text[p:p + n], dw.Stream(), 0
        cuts = sorted({len(piece)} | {int(rng.integers(0, len(piece) + 1)) for _ in range(int(rng.integers(0, 4)))})
        for i, e in enumerate(cuts):
            final, kind = i + 1 == len(cuts), int(rng.integers(0, 3))
            toks = dw.tokenize(piece[q:e], piece[:q], min_match=int(rng.integers(3, 8)), max_dist=int(rng.choice([4, 300, 5000, 32768])),
                               max_len=int(rng.choice([3, 10, 64, 258])))
            if kind == 0:
                s.stored(piece[q:e], final)
            elif kind == 1:
                s.fixed(toks, final)
            else:
                fl, fd = dw.symbol_freqs(toks)
                nd = sum(1 for x in fd if x)
                dist = dw.no_codes() if nd == 0 else dw.one_code(fd.index(max(fd)), 30) if nd == 1 else noisy_lengths(fd)
                s.dynamic(toks, noisy_lengths(fl), dist, final, cl_plan={"mode": str(rng.choice(["literal", "greedy", "split"]))})
            q = e
        assert zlib.decompress(s.bytes(), -15) == piece, "the writer and zlib disagree"
        parts.append(dw.bgzf_block(s.bytes(), piece))
        p += n
        if rng.random() < 0.02:
            parts.append(dw.BGZF_EOF)
    if rng.random() < 0.7:
        parts.append(dw.BGZF_EOF)
    offs, o = [], 0
    for b in parts:
        offs.append((o, len(b))); o += len(b)
    return b"".join(parts), offs


def fuzz_bgzf():
    import struct
    written = "written" in sys.argv[1:]
    os.environ["SHK_GUNZIP_DEVICE_MIN"] = "0"                # (every file, however small)
    t0 = time.time()
    reasons = Counter()
    for case in range(n_cases):
        text = fg.make_text(int(rng.choice([70000, 300_000] if written else [70000, 300_000, 3_000_000, 8_000_000])))
        z, offs = written_bgzf_file(text) if written else bgzf_file(text)
        # at times through the windows of the large-file route: text per window from one block's worth up (csrc/preprocess.cpp, route 2)
        os.environ.pop("SHK_GUNZIP_DEVICE_WINDOW", None)
        if rng.random() < 0.5:
            os.environ["SHK_GUNZIP_DEVICE_WINDOW"] = str(int(rng.choice([65536, 100000, 1 << 20, 5 << 20])))
        desc = dict(case=case, size=len(text), zlen=len(z), blocks=len(offs), window=os.environ.get("SHK_GUNZIP_DEVICE_WINDOW"))
        try:
            rc, got, why, _ = device_gunzip(z)
            assert rc == 0, ("an intact BGZF file was not taken", rc, why)
            assert got == text, ("intact file: OTHER BYTES", len(got), len(text))
            bads = [z[:int(rng.integers(1, len(z)))], z[:-1], z + b"\0"]
            for _ in range(3):
                pos = int(rng.integers(0, len(z)))
                bad = bytearray(z); bad[pos] ^= 1 << int(rng.integers(0, 8)); bads.append(bytes(bad))
            for _ in range(3):                               # a header or trailer field of one block: BSIZE, CRC-32, ISIZE
                o, bs = offs[int(rng.integers(0, len(offs)))]
                at, fmt = [(o + 16, "<H"), (o + bs - 8, "<I"), (o + bs - 4, "<I")][int(rng.integers(0, 3))]
                old = struct.unpack_from(fmt, z, at)[0]
                new = max(0, old + int(rng.choice([-1, 1, 1000, 70000]))) & (0xFFFF if fmt == "<H" else 0xFFFFFFFF)
                bad = bytearray(z); struct.pack_into(fmt, bad, at, new); bads.append(bytes(bad))
            for bad in bads:
                rc2, got2, why2, _ = device_gunzip(bad)
                assert rc2 in (0, 1), ("error code", rc2, why2)
                if rc2 == 0:
                    rch, goth, _ = fg.gunzip(bad)
                    assert rch == 0 and got2 == goth, ("damaged file: not the host reader's bytes", rch)
                else:
                    reasons[why2] += 1
        except Exception as e:
            print("FAIL", desc, repr(e), flush=True)
            raise
        if case % 10 == 0:
            print("case", case, "ok  %.0f s" % (time.time() - t0), flush=True)
    print("all", n_cases, "BGZF cases: every intact file taken with its bytes; damaged ones declined or as the host reads them; declined:", dict(reasons),
          "; %.0f s" % (time.time() - t0))


if "bgzf" in sys.argv[1:]:
    fuzz_bgzf()
    sys.exit(0)

t0 = time.time()
taken, reasons, rates = 0, Counter(), []
for case in range(n_cases):
    n_members = int(rng.choice([1, 1, 1, 1, 2]))
    size = int(rng.choice([70000, 300_000, 3_000_000, 8_000_000, 20_000_000]))
    os.environ["SHK_GUNZIP_DEVICE_CHUNK"] = str(int(rng.choice([4096, 16384, 49152, 49152, 200000])))
    members, texts, descs = [], [], []
    for _ in range(n_members):
        t = fg.make_text(size)
        z, d = fg.compress(t)
        members.append(z); texts.append(t); descs.append(d)
    z, want = b"".join(members), b"".join(texts)
    desc = dict(case=case, members=n_members, size=size, zlen=len(z), chunk=os.environ["SHK_GUNZIP_DEVICE_CHUNK"], how=descs)
    try:
        rc, got, why, ms = device_gunzip(z)
        assert rc in (0, 1), ("error code", rc, why)
        if rc == 0:
            assert n_members == 1, "several members taken as one"
            assert got == want, ("intact stream: OTHER BYTES", len(got), len(want))
            taken += 1
            if len(want) >= 3_000_000:
                rates.append(len(want) / 1e9 / (ms * 1e-3))
        else:
            reasons[why] += 1
        # damaged streams: declined, or (harmless damage) zlib's bytes
        for cut in (int(rng.integers(1, len(z))), len(z) - 1, len(z) - 8):
            if 0 < cut < len(z):
                rc2, got2, why2, _ = device_gunzip(z[:cut])
                assert rc2 == 1 or (rc2 == 0 and got2 == fg.zlib_gunzip(z[:cut])), ("truncated at", cut, rc2)
        for _ in range(3):
            pos = int(rng.integers(2, len(z)))
            bad = bytearray(z); bad[pos] ^= 1 << int(rng.integers(0, 8)); bad = bytes(bad)
            try:
                ref = fg.zlib_gunzip(bad)
            except zlib.error:
                ref = None
            rc2, got2, why2, _ = device_gunzip(bad)
            assert rc2 == 1 or (rc2 == 0 and ref is not None and got2 == ref), ("corrupt byte at", pos, rc2, "zlib error" if ref is None else "zlib fine")
    except Exception as e:
        print("FAIL", desc, repr(e), flush=True)
        raise
    if case % 10 == 0:
        print("case", case, "ok  %.0f s" % (time.time() - t0), "taken so far", taken, flush=True)
print("all", n_cases, "cases: zlib's bytes, or declined; the device inflater took", taken, "intact members; declined:", dict(reasons),
      "; GB/s of text on the members >= 3 MB it took: min %.2f median %.2f max %.2f" % (min(rates), sorted(rates)[len(rates) // 2], max(rates)) if rates else "",
      "; %.0f s" % (time.time() - t0))
