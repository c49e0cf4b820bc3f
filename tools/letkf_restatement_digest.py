#!/usr/bin/env python3
"""SHA-256 digests of what the tests' NumPy restatement of the ensemble analysis computes (tests/letkf.py and the letkf* modules
next to it), on the CPU: run on the tests directory of an earlier commit and on this one, every digest must be equal.  The
restatement is what every LETKF test compares the device with, so a change in it that moves a bit moves the yardstick; the tests
would not notice.  profiles/letkf_restatement_digests.json keeps both rows of the change that stated the analysis call once.

A record, not a test: NumPy's arcsin and einsum need not give the same bits on another machine or version, so both rows are made
on one machine and nothing in tests/ reads the file.

T30 L8 and T30 L5 host-only plans, E = 2, 5, 32, sigma_v = 0 and 0.3, at tests/letkf.py's columns_for.  Per combination: the level
network edge_obs + clustered_obs(n=300) + sparse_obs; letkfpressure.network on craft; both from three slots on drifting; both
with two members dropped (E >= 5); the level network with values planted around the background check's threshold and
letkfqc.check's r_eff; the level network at weight stride (2, 2).  Digests: the obs-space dict, C and b, the increments by eigh and
by Jacobi, letkfinfl.sums and update, letkfrelax.relax.  An earlier tests directory is read through the functions it had (the
five forms of `problems`, the tuple of letkf.obs_space); this one through letkf.obs_space and letkf.problems alone.

    python tools/letkf_restatement_digest.py --label this [--json out.json]
    python tools/letkf_restatement_digest.py --tests /path/to/earlier/tests --label parent"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGMA_V, MEMBERS, PLANS, SEED, GROSS = (0.0, 0.3), (2, 5, 32), ("t30", "t30k5"), 60, 3.0
LEVEL, FIELDS = ("hx", "hxmean", "y", "departure"), ("hx", "hxmean", "y", "departure", "obs_lnsigma", "obs_used")


def sha(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, np.float64).tobytes())
    return h.hexdigest()


def restate(m, g, x, obs, sigma_v, cols, keep=None, xs=None, first=None, r_eff=None):
    """-> (the obs-space dict, C, b) by the functions the tests directory has"""
    lk, n = m["lk"], len(obs["var"])
    if hasattr(lk, "couple"):
        s = lk.obs_space(g, x, obs, keep, xs=xs, first=first)
        return (s,) + lk.problems(g, obs, s, lk.SIGMA_H, sigma_v, cols, keep, r_eff)
    if xs is not None or keep is not None:
        C, b, s = m["ls"].problems_slots(g, xs or [x], obs, first or [0, n], lk.SIGMA_H, sigma_v, cols, keep)
    elif "p" in obs:
        s = m["lp"].obs_space(g, x, obs)
        C, b = m["lp"].problems(g, x, obs, lk.SIGMA_H, sigma_v, cols)
    else:
        s = dict(zip(LEVEL, lk.obs_space(g, x, obs)), obs_lnsigma=lk.lnsigma(g, obs), obs_used=np.ones(n))
        if r_eff is not None:
            C, b = m["qc"].problems(g, x, obs, r_eff, lk.SIGMA_H, sigma_v, cols)
        else:
            C, b = lk.problems(g, x, obs, lk.SIGMA_H, sigma_v, cols)
            Cl, bl = lk.local_problems(g, x, obs, lk.SIGMA_H, sigma_v, cols)
            assert sha([C, b]) == sha([Cl, bl]), "the earlier problems and local_problems differ"
    return s, C, b


def case(m, out, tag, g, x, obs, sigma_v, cols, fields, keep=None, **how):
    """the digests of one analysis call under out[tag + ...]"""
    lk, li, lr = m["lk"], m["li"], m["lr"]
    s, C, b = restate(m, g, x, obs, sigma_v, cols, keep, **how)
    out[tag + " obs_space"], out[tag + " C b"] = sha([s[n] for n in fields]), sha([C, b])
    xk = x if keep is None else {v: np.ascontiguousarray(x[v][sorted(keep)]) for v in lk.VARS}
    inc = {}
    for route in ("eigh", "jacobi"):
        inc[route], _ = lk.increments(g, xk, C, b, lk.RHO, route, cols)
        out[tag + " increments " + route] = sha([inc[route][v] for v in lk.VARS])
    rinv = how.get("r_eff")
    rinv = s["obs_used"] / (obs["error"] * obs["error"]) if rinv is None else rinv
    p = li.sums(g, lk.unit(obs["lon"], obs["lat"]), s["obs_lnsigma"], rinv, s["departure"], li.s2(s["y"], keep), lk.SIGMA_H, sigma_v, cols)
    out[tag + " infl sums update"] = sha([p, li.update(np.full(p.shape[1:], lk.RHO), p, 0.5)])
    dx, f = lr.relax({v: lk.at_columns(xk[v], cols) for v in lk.VARS}, inc["eigh"], 0.3, 0.9)
    out[tag + " relax"] = sha([dx[v] for v in lk.VARS] + [f[v] for v in lk.VARS])


def digests(m):
    lk, lp, ls, qc, li = (m[n] for n in ("lk", "lp", "ls", "qc", "li"))
    out = {}
    for plan in PLANS:
        sp = m["support"].plan(plan, 32 * 17, device=-1)
        g = lp.Geometry(sp)
        for E in MEMBERS:
            x, xp = lk.ensemble(g, E, SEED + E), lp.craft(g, E, SEED + E)
            level = lk.concat(lk.edge_obs(g, x), lk.clustered_obs(g, x, n=300), lk.sparse_obs(g, x))
            nets = (("level", x, level, LEVEL), ("pressure", xp, lp.network(g, xp), FIELDS))
            for sigma_v in SIGMA_V:
                for kind, y, obs, fields in nets:
                    tag = "%s E=%d sigma_v=%g %s" % (plan, E, sigma_v, kind)
                    cols, n = lk.columns_for(g, obs, lk.SIGMA_H), len(obs["var"])
                    first, ys = [0, 1, 300, n], ls.drifting(g, y, 3, SEED + 7)
                    case(m, out, tag, g, y, obs, sigma_v, cols, fields)
                    case(m, out, tag + " slots", g, y, obs, sigma_v, cols, FIELDS + ("slot_ps", "slot_out"), xs=ys, first=first)
                    if E >= 5:
                        keep = [e for e in range(E) if e not in (1, E - 2)]
                        case(m, out, tag + " mask", g, y, obs, sigma_v, cols, FIELDS, keep)
                        case(m, out, tag + " mask slots", g, y, obs, sigma_v, cols, FIELDS + ("slot_ps", "slot_out"), keep, xs=ys, first=first)
                tag, cols = "%s E=%d sigma_v=%g" % (plan, E, sigma_v), lk.columns_for(g, level, lk.SIGMA_H)
                s, _, _ = restate(m, g, x, level, sigma_v, cols[:1])
                planted = dict(level, value=qc.plant(level, s["hxmean"], qc.spread2(s["y"]), GROSS, SEED)[0])
                s, _, _ = restate(m, g, x, planted, sigma_v, cols[:1])
                dec = qc.check(s["y"], s["departure"], planted["error"], GROSS)
                assert dec["rej"].any() and dec["used"].any()
                case(m, out, tag + " qc", g, x, planted, sigma_v, cols, LEVEL, r_eff=qc.reff(dec["used"], 1.0 / (planted["error"] * planted["error"])))
                for route in ("eigh", "jacobi"):
                    inc, _, Tc = m["lx"].analyse(g, x, level, lk.SIGMA_H, sigma_v, lk.RHO, 2, 2, route, cols)
                    out[tag + " stride (2, 2) " + route] = sha([inc[v] for v in lk.VARS] + [Tc])
        sp.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tests", default=os.path.join(ROOT, "tests"), help="the tests directory to read the restatement from")
    ap.add_argument("--label", default="this")
    ap.add_argument("--json")
    a = ap.parse_args()
    sys.path[:0] = [ROOT, os.path.abspath(a.tests)]
    import importlib
    names = {"lk": "letkf", "lp": "letkfpressure", "ls": "letkfslots", "qc": "letkfqc", "li": "letkfinfl", "lr": "letkfrelax",
             "lx": "letkfinterp", "support": "support"}
    m = {k: importlib.import_module(v) for k, v in names.items()}
    assert os.path.dirname(os.path.abspath(m["lk"].__file__)) == os.path.abspath(a.tests)
    m["support"].package()
    row = {"label": a.label, "numpy": np.__version__, "digests": digests(m)}
    print(json.dumps(row, indent=1))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(row, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
