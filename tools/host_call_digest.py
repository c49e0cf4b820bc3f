#!/usr/bin/env python3
"""SHA-256 digests of what every host-pointer entry point returns: run once on an earlier build's library
($SPDY_LIB) and once on this one, every digest must be equal.  The tests in the tree compare one route or one form of a build with
another of the same build; a change in the layer they share -- the staging of a call's host arrays (csrc/spdy_plan.hpp,
spdy_detail::HostCall) -- that moved the same wrong bytes on both routes would pass them all and shows here.

The cases, inputs and sizes are those of tests/hostcalls.py: T30 and T63, kx = 8, max_batch = 16; one digest per (resolution, entry
point, size, route) over every output array of the call, the outputs handed in filled with a fixed pattern.  Routes: "device"
(SPDY_HOST_STAGE_KB=0) and "default" (small calls through host-mapped staging).

    python tools/host_call_digest.py [--label l] [--json out.json]
    SPDY_LIB=/path/to/earlier/libspdy.so python tools/host_call_digest.py --label parent"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import hostcalls as hc  # noqa: E402
import speedy_f90_amd as s  # noqa: E402


def sha(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="this build")
    ap.add_argument("--json")
    a = ap.parse_args()
    out = {}
    for tag in ("t30", "t63"):
        for route, kb in hc.ROUTES.items():
            os.environ.pop("SPDY_HOST_STAGE_KB", None)
            if kb is not None:
                os.environ["SPDY_HOST_STAGE_KB"] = kb
            sp = hc.plan(tag)
            d = hc.Data(sp)
            for case in hc.CASES:
                for nb in hc.sizes(case):
                    rc, outs = hc.run_host(sp, case, hc.arguments(case, d, nb))
                    if rc:
                        raise SystemExit("%s %s n=%s on route %s: return code %d" % (tag, case, nb, route, rc))
                    out["%s %s n=%s %s" % (tag, case, nb, route)] = sha(outs)
            sp.close()
    row = {"label": a.label, "library": os.path.basename(os.path.dirname(s.LIB_PATH)) + "/" + os.path.basename(s.LIB_PATH), "digests": out}
    print(json.dumps(row, indent=1), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(row, f, indent=1)


if __name__ == "__main__":
    main()
