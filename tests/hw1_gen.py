"""Seeded hw1 inputs (references + reads) that any machine regenerates byte for byte: a 64-bit LCG over 4096 lanes in numpy
(uint64 arithmetic wraps), no library random stream; and the reference's readSequences restated.  Used by
tests/golden/make_golden_hw1.py, the hw1 tests and tools/hw1_scale.py."""
import numpy as np

LANES = 4096
_A, _C = np.uint64(6364136223846793005), np.uint64(1442695040888963407)


def lcg_u32(seed, count):
    """count uint32 values of stream `seed`"""
    steps = -(-count // LANES)
    s = (np.arange(LANES, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) ^ np.uint64(seed * 0x2545F4914F6CDD1D % (1 << 64))
    out = np.empty((max(steps, 1), LANES), dtype=np.uint32)
    with np.errstate(over="ignore"):
        for _ in range(4):   # decorrelate the lanes' starting points
            s = s * _A + _C
        for k in range(steps):
            s = s * _A + _C
            out[k] = (s >> np.uint64(32)).astype(np.uint32)
    return out.reshape(-1)[:count]


def dna(seed, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[lcg_u32(seed, n) & 3].tobytes()


def genome(seed, total, n_refs):
    """n_refs references of about total / n_refs bases each, headers chr00, chr01, ..."""
    u = lcg_u32(seed, n_refs)
    base = total // n_refs
    lens = [max(200, base + int(x % 2001) - 1000) for x in u]
    return [(b"chr%02d" % i, dna(seed * 1000 + i + 1, m)) for i, m in enumerate(lens)]


def reads(seed, refs, n, lo=20, hi=100):
    """n reads of lo..hi bases: exact substrings, one in ten with one base changed, one in fifty random"""
    u = lcg_u32(seed, 4 * n).reshape(n, 4)
    rnd = dna(seed + 7, hi * 64)
    out = []
    for k in range(n):
        r = refs[int(u[k, 0]) % len(refs)][1]
        m = lo + int(u[k, 1]) % (hi - lo + 1)
        if k % 50 == 49:
            o = int(u[k, 2]) % (len(rnd) - m)
            s = rnd[o:o + m]
        else:
            p = int(u[k, 2]) % (len(r) - m)
            s = r[p:p + m]
            if k % 10 == 3:
                i = int(u[k, 3]) % m
                s = s[:i] + bytes([b"ACGT"[(b"ACGT".index(s[i]) + 1 + int(u[k, 3]) % 3) % 4]]) + s[i + 1:]
        out.append((b"read%d" % k, s))
    return out


def read_sequences(data):
    """readSequences of the hw1 reference, restated over bytes: stop at the first empty line, trim " \\t\\r\\n", keep records
    with a non-empty header, clear the sequence only when a record is kept"""
    recs, header, seq = [], b"", b""
    for line in data.split(b"\n") if data else []:
        if line == b"":
            break
        line = line.strip(b" \t\r\n")
        if line[:1] == b">":
            if header:
                recs.append((header, seq))
                seq = b""
            header = line[1:]
        else:
            seq += line
    if header:
        recs.append((header, seq))
    return recs


def fasta(records, width=80):
    parts = []
    for h, s in records:
        parts.append(b">" + h + b"\n")
        for i in range(0, len(s), width):
            parts.append(s[i:i + width] + b"\n")
    return b"".join(parts)
