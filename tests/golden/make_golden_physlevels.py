#!/usr/bin/env python3
"""Regenerate tests/golden/ref_physlevels.npz: the REAL reference's column physics at the level counts of tests/physlevels.py
(6, 9, 12, 15 at T30, on tests/levels.py's half levels; build container only).

One flang build per count, make_golden_surface.py's (the reference modules compiled where they lie with `kx` edited by sed into a
mktemp directory that is deleted afterwards; the committed shims are the bind(C) entries; the half levels go in through
moist_init(have_levels = 1, ...), since the reference has no set for any of these counts).  On it run, as they are, the run() of
make_golden_moist.py, make_golden_radiation.py and make_golden_surface.py, and at 12 levels make_golden_thresholds.py's on
thresholds.build's constructed columns.  Their keys go into one file under the prefixes "moist_", "rad_", "sfc_" and "thr_", with
smaller column samples than the four-variant fixtures keep (every branch is still in each).  Nothing from the reference is
committed: the only output is the npz.

    python tests/golden/make_golden_physlevels.py
"""
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import make_golden_moist as mg  # noqa: E402
import make_golden_radiation as mr  # noqa: E402
import make_golden_surface as ms  # noqa: E402
import make_golden_thresholds as mt  # noqa: E402
import physlevels  # noqa: E402

NUNIFORM, NBRANCH = 16, 2


def main():
    if not (os.path.isdir(mg.REF) and os.access(mg.FC, os.X_OK)):
        sys.exit("make_golden_physlevels: needs the reference sources ($SPEEDY_REFERENCE) and flang")
    tmp = tempfile.mkdtemp(prefix="spdy_lev_")
    d, done = {}, []

    def work():
        for tag in physlevels.TAGS:
            lib = ms.build(tag, tmp)
            for pre, mod in (("moist_", mg), ("rad_", mr), ("sfc_", ms)):
                d.update({pre + k: v for k, v in mod.run(tag, lib, NUNIFORM, NBRANCH).items()})
            if physlevels.kx_of(tag) == physlevels.THRESHOLD_COUNT:
                t = mt.run(tag, lib, seed=physlevels.THRESHOLD_SEED)
                d.update({"thr_" + k: v for k, v in t.items() if "_year" not in k and "_tyear" not in k})
            done.append(tag)
    import threading
    threading.stack_size(256 << 20)
    th = threading.Thread(target=work)
    try:
        th.start()
        th.join()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    if len(done) < len(physlevels.TAGS):
        sys.exit("make_golden_physlevels: a variant failed")
    out = os.path.join(HERE, "ref_physlevels.npz")
    np.savez_compressed(out, **d)
    print("wrote %s (%.2f MB)" % (out, os.path.getsize(out) / 1e6))


if __name__ == "__main__":
    main()
