#!/usr/bin/env python3
"""SHA-256 digests of what the observation stage of the ensemble analysis and the nature run's draws compute: run
once on an earlier build's library ($SPDY_LIB) and once on this one, every digest must be equal.  The tests in the tree compare
one path of a build with another path of the same build; a change made in the operator they share (csrc/spdy_obsop.hpp) -- another
association of the bilinear sum, say -- would pass them all and shows here.

T30 L8, fixed seeds, the networks of tests/letkf.py (model levels) and tests/letkfpressure.py (observations at a pressure), each
case for E = 5 (odd, padded, does not divide a workgroup) and E = 32: the analysis plain, under a mask that drops two members, from
three time slots observed on the same ensemble, and at weight stride (2, 2); digest over hx, hxmean, y, departure, obs_lnsigma,
obs_used, value and the five increments.  Nature.observe: the whole network and slot by slot, noise 0 and 1; digest over value.

    python tools/letkf_digest.py [--json out.json]
    SPDY_LIB=/path/to/earlier/libspdy.so python tools/letkf_digest.py --earlier-library --label parent"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import letkf as lk  # noqa: E402
import letkfpressure as lp  # noqa: E402
import letkfslots as ls  # noqa: E402
import support  # noqa: E402
import speedy_f90_amd as s  # noqa: E402

FIELDS = ("hx", "hxmean", "y", "departure", "obs_lnsigma", "obs_used", "value")
MEMBERS, SIGMA_V, SEED = (5, 32), 0.3, 40


def sha(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, np.float64).tobytes())
    return h.hexdigest()


def analysis(lt, x, **how):
    """the call and its digest, by the library's calls alone: the tool also serves the tests directory of an earlier commit"""
    import torch
    inc = lt.analyse_grid(*[support.dev(x[v]) for v in lk.VARS], **how)
    torch.cuda.synchronize()
    return sha([lt.field(n).numpy() for n in FIELDS] + [a.cpu().numpy() for a in inc])


def networks(g, E):
    """(kind, ensemble, network, maker) of the two kinds; about 700 and 600 observations: more than one workgroup in every layout"""
    x = lk.ensemble(g, E, SEED + E)
    level = lk.concat(lk.edge_obs(g, x), lk.clustered_obs(g, x, n=600), lk.sparse_obs(g, x))
    xp = lp.craft(g, E, SEED + E)
    return (("level", x, level, lk.make), ("pressure", xp, lp.network(g, xp), lp.make))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="this build")
    ap.add_argument("--json")
    ap.add_argument("--earlier-library", action="store_true", help="$SPDY_LIB is from before this build's newest entry points")
    a = ap.parse_args()
    if a.earlier_library:                 # bind without what it lacks; nothing here calls it
        import ctypes
        raw = ctypes.CDLL(s._lib.LIB_PATH)
        for n in [n for n in s._lib.SIGNATURES if not hasattr(raw, n)]:
            del s._lib.SIGNATURES[n]
    sp = support.ensemble_plan("t30", max(MEMBERS))
    g = lp.Geometry(sp)
    out = {}
    for E in MEMBERS:
        use = [1] * E
        use[1] = use[E - 2] = 0
        for kind, x, net, make in networks(g, E):
            n = len(net["var"])
            first = [0, n // 3, 2 * n // 3, n]
            for stride in ((1, 1), (2, 2)):
                lt = make(sp, E, net, SIGMA_V)
                if stride != (1, 1):
                    lt.set_weight_stride(*stride)
                tag = "%s E=%d%s" % (kind, E, "" if stride == (1, 1) else " stride 2 2")
                out[tag + " plain"] = analysis(lt, x)
                out[tag + " masked"] = analysis(lt, x, use=use)
                if stride == (1, 1):
                    ls.observe_all(lt, [x] * 3, first)
                    out[tag + " slots plain"] = analysis(lt, x, slots=True)
                    out[tag + " slots masked"] = analysis(lt, x, slots=True, use=use)
                lt.close()
            if E != MEMBERS[0]:
                continue
            # the nature run: the truth is member 0 of the kind's ensemble
            lt, nat = make(sp, E, net, SIGMA_V), s.Nature(sp, seed=SEED)
            nat.field("truth").upload(np.concatenate([x[v][0] for v in lk.VARS[:4]] + [x["ps"][0][None]]))
            for noise in (0.0, 1.0):
                nat.reset(SEED)
                lt.set_slots(None)
                nat.observe(lt, noise)
                out["nature %s noise %g whole" % (kind, noise)] = sha([lt.field("value").numpy()])
                nat.reset(SEED)
                lt.set_slots(first)
                for k in range(3):
                    nat.observe(lt, noise, slot=k)
                out["nature %s noise %g slots" % (kind, noise)] = sha([lt.field("value").numpy()])
            nat.close()
            lt.close()
    sp.close()
    row = {"label": a.label, "library": os.path.basename(os.path.dirname(s.LIB_PATH)) + "/" + os.path.basename(s.LIB_PATH), "digests": out}
    print(json.dumps(row, indent=1), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(row, f, indent=1)


if __name__ == "__main__":
    main()
