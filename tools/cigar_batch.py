"""CIGAR / MD:Z of whole batches: pwa_align_batch + the host formatter loop against pwa_align_batch_cigar.

For each shape, whole-call wall times over --reps repetitions (median and min..max), after one warm-up call:
  (a) pwa_align_batch, then pwa_format_alignment on every pair through ctypes (the loop a Python caller writes), and
      the same loop with n_ops = 0 (argument marshalling and the call itself: the loop's ctypes share);
  (b) pwa_align_batch_cigar;
  (c) device ms of the fills and the walks (pwa_align_last_stats, event-timed);
      the count / scan / write kernels: from a rocprofv3 --kernel-trace --stats run of this script;
  (d) device-to-host bytes: the op regions pwa_align_batch copies back against the packed strings + offsets.
Both calls' strings are compared byte for byte on every repetition's last call.

    python tools/cigar_batch.py [--reps 5] [--shapes g,reads,long] [--json out.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as G  # noqa: E402


def gen_dna(rng, n):
    return rng.choice(np.frombuffer(b"ACGT", np.uint8), n)


def mutate(rng, s, rate):
    """substitutions, insertions and deletions, each at about rate / 3 per symbol"""
    s = s.copy()
    sub = rng.random(len(s)) < rate / 3
    s[sub] = gen_dna(rng, int(sub.sum()))
    at = np.flatnonzero(rng.random(len(s)) < rate / 3)
    s = np.insert(s, at, gen_dna(rng, len(at)))
    return s[rng.random(len(s)) >= rate / 3].tobytes()


def shape(name, rng):
    if name == "g":   # hw2 -g over 64 texts of 10k: 4096 NW pairs of 150 x 10k
        texts = [gen_dna(rng, 10000).tobytes() for _ in range(64)]
        pats = [gen_dna(rng, 150).tobytes() for _ in range(64)]
        return "nw", (1, -1, -1), pats + texts, [i % 64 for i in range(4096)], [64 + i // 64 for i in range(4096)]
    if name == "reads":   # 65 536 local pairs: 150-symbol reads from 1000-symbol windows at ~3 % divergence
        seqs, pa, pb = [], [], []
        for k in range(65536):
            win = gen_dna(rng, 1000)
            at = int(rng.integers(0, 850))
            seqs += [mutate(rng, win[at:at + 150], 0.03), win.tobytes()]
            pa.append(2 * k)
            pb.append(2 * k + 1)
        return "sw", (2, -3, -5), seqs, pa, pb
    if name == "long":   # 64 NW pairs of 10k x 10k (mutated copies)
        seqs = []
        for _ in range(64):
            a = gen_dna(rng, 10000)
            seqs += [a.tobytes(), mutate(rng, a, 0.05)]
        return "nw", (1, -1, -1), seqs, list(range(0, 128, 2)), list(range(1, 128, 2))
    raise ValueError(name)


def med(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), n=len(xs))


def run(ctx, L, name, reps, rng):
    pkg = G.load_pkg()
    mode, sc, seqs, pa_l, pb_l = shape(name, rng)
    blob, off, seqs = pkg.pack_sequences(seqs)
    n = len(pa_l)
    pa = np.array(pa_l, np.uint32)
    pb = np.array(pb_l, np.uint32)
    lens = np.array([len(s) for s in seqs], np.uint64)
    nm = lens[pa] + lens[pb]
    u32p, u64p, i32p, vp = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_int32), C.c_void_p
    m = pkg.MODE[mode]
    # pwa_align_batch's buffers: one tiled op region per pair (the single-copy layout)
    ops_off = np.zeros(n, np.uint64)
    ops_off[1:] = np.cumsum(nm[:-1])
    ops = np.zeros(int(nm.sum()) + 1, np.uint8)
    scores = np.zeros(n, np.int32)
    n_ops = np.zeros(n, np.uint64)
    endc = np.zeros(2 * n, np.uint64)
    startc = np.zeros(2 * n, np.uint64)
    # pwa_align_batch_cigar's: the bounds
    cap_c, cap_m = int((2 * nm + 24).sum()), int((3 * nm + 24).sum())
    cg, md = np.zeros(cap_c, np.uint8), np.zeros(cap_m, np.uint8)
    cg_off, md_off = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint64)
    scores2 = np.zeros(n, np.int32)

    def align_batch():
        rc = L.pwa_align_batch(ctx._h, m, *sc, blob, off, len(seqs), pa.ctypes.data_as(u32p), pb.ctypes.data_as(u32p), n,
                               scores.ctypes.data_as(i32p), ops.ctypes.data_as(vp), ops_off.ctypes.data_as(u64p),
                               n_ops.ctypes.data_as(u64p), endc.ctypes.data_as(u64p), startc.ctypes.data_as(u64p))
        assert rc == 0, rc

    def align_batch_cigar():
        rc = L.pwa_align_batch_cigar(ctx._h, m, *sc, blob, off, len(seqs), pa.ctypes.data_as(u32p), pb.ctypes.data_as(u32p), n,
                                     scores2.ctypes.data_as(i32p), cg.ctypes.data_as(vp), cap_c, cg_off.ctypes.data_as(u64p),
                                     md.ctypes.data_as(vp), cap_m, md_off.ctypes.data_as(u64p), None, None, None)
        assert rc == 0, rc

    # the per-pair formatter loop: buffers sized for the longest pair, reused
    mx = int(nm.max())
    ap, ar = C.create_string_buffer(mx + 1), C.create_string_buffer(mx + 1)
    cgb, mdb = C.create_string_buffer(3 * mx + 24), C.create_string_buffer(3 * mx + 24)
    ov = C.c_int32(0)
    seq_ptr = [C.c_void_p(C.cast(C.c_char_p(blob), C.c_void_p).value + int(off[s])) for s in range(len(seqs))]
    base = ops.ctypes.data
    f_cig, f_mdz = [], []

    def format_loop(empty=False, keep=False):
        endp = (C.c_uint64 * 2)()
        for k in range(n):
            a, b = pa_l[k], pb_l[k]
            endp[0], endp[1] = int(endc[2 * k]), int(endc[2 * k + 1])
            cnt = 0 if empty else int(n_ops[k])
            rc = L.pwa_format_alignment(seq_ptr[a], int(lens[a]), seq_ptr[b], int(lens[b]), C.c_void_p(base + int(ops_off[k])), cnt,
                                        endp, ap, ar, cgb, mdb, C.byref(ov))
            assert rc == 0
            if keep:
                f_cig.append(cgb.value)
                f_mdz.append(mdb.value)

    t_ab, t_fmt, t_empty, t_cig = [], [], [], []
    fill, walk = [], []
    align_batch()
    align_batch_cigar()
    for r in range(reps):
        t0 = time.perf_counter()
        align_batch()
        t1 = time.perf_counter()
        format_loop(keep=(r == reps - 1))
        t2 = time.perf_counter()
        format_loop(empty=True)
        t3 = time.perf_counter()
        align_batch_cigar()
        t4 = time.perf_counter()
        fm, wm, bb = C.c_float(0), C.c_float(0), C.c_uint64(0)
        L.pwa_align_last_stats(ctx._h, C.byref(fm), C.byref(wm), C.byref(bb))
        t_ab.append((t1 - t0) * 1e3)
        t_fmt.append((t2 - t1) * 1e3)
        t_empty.append((t3 - t2) * 1e3)
        t_cig.append((t4 - t3) * 1e3)
        fill.append(fm.value)
        walk.append(wm.value)
    # the two paths agree (scores and every string)
    assert (scores == scores2).all()
    cgs, mds = cg.tobytes(), md.tobytes()
    same = all(cgs[int(cg_off[k]):int(cg_off[k + 1])] == f_cig[k] and mds[int(md_off[k]):int(md_off[k + 1])] == f_mdz[k] for k in range(n))
    assert same, "strings differ between the two paths"
    a_whole = [x + y for x, y in zip(t_ab, t_fmt)]
    out = dict(shape=name, mode=mode, scoring=sc, pairs=n, cells=int((lens[pa] * lens[pb]).sum()),
               a_align_batch_plus_format_ms=med(a_whole), a_align_batch_ms=med(t_ab), a_format_loop_ms=med(t_fmt),
               a_format_loop_ctypes_only_ms=med(t_empty), b_align_batch_cigar_ms=med(t_cig),
               c_fill_ms=med(fill), c_walk_ms=med(walk),
               d_ops_bytes=int(nm.sum()), d_strings_bytes=int(cg_off[n] + md_off[n]), d_offset_bytes=int((2 * n + 2) * 4),
               op_columns=int(n_ops.sum()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="g,reads,long")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    pkg = G.load_pkg()
    L = pkg.lib()
    ctx = pkg.Context(0)
    rng = np.random.default_rng(20261016)
    res = []
    for name in args.shapes.split(","):
        r = run(ctx, L, name, args.reps, rng)
        print(json.dumps(r), flush=True)
        res.append(r)
    ctx.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
