"""Device time of batched SW scores for short patterns on the packed profile form: 4096 patterns of 100 and of 150 rows against the
c3 texts (256 of 10 kbp), Context.batch("sw", ...).run_times() over a few runs.  One JSON line per pattern length.
    python tools/profile_rows_time.py [--root DIR]      (DIR: another built checkout of this repository, e.g. the parent commit)"""
import argparse
import importlib.util
import json
import os
import sys

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
ap.add_argument("--runs", type=int, default=5)
args = ap.parse_args()
root = os.path.abspath(args.root)
sys.path.insert(0, os.path.join(root, "tests"))
spec = importlib.util.spec_from_file_location("graft_entry", os.path.join(root, "__graft_entry__.py"))
entry = importlib.util.module_from_spec(spec)
spec.loader.exec_module(entry)
import oracle_lib as O

pkg = entry.load_pkg()
ctx = pkg.Context(0)
txts = [O.gen(1, 1, t, 10000) for t in range(256)]
pa = np.repeat(np.arange(4096, dtype=np.uint32), 256)
pb = np.tile(np.arange(256, dtype=np.uint32) + np.uint32(4096), 4096)
for n in (100, 150):
    pats = [O.gen(1, 0, p, n) for p in range(4096)]
    b = ctx.batch("sw", pats + txts, pa, pb, 1, -1, -1)
    for _ in range(args.runs + 1):
        b.run()
    ms = b.run_times()[1:]   # (the first run is the warm-up)
    s = b.fetch(numpy_out=True)
    info = b.info()
    print(json.dumps(dict(rows=n, profile_form=b.profile_form(), profile_int=b.profile_int(), ms=[round(x, 3) for x in ms], ms_min=round(min(ms), 3),
                          checksum=int(s.astype(np.int64).sum()), padded_cells=info["padded_cells"], cells=info["cells"], root=os.path.basename(root))))
    b.close()
ctx.close()
