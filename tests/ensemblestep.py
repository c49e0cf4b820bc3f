"""What the ensemble tests share: members with DIFFERENT states (distinct seeds of dynstep.state; equal members would prove nothing
about addressing), the ensemble built from them, a member's part of an ensemble snapshot in the single state's layout, and the
single-state run (modelstep.step) that every member is compared with."""
import numpy as np

import levels
import modelstep
import moist
import physstep
import support
from dynstep import ROB
from dynstep import state as dyn_state

PROG = ("vor", "div", "t", "tr", "ps")
COMPARED = PROG + ("phi", "U", "V", "PL")
LEAPFROG = ((2, 2, 1.0), (2, 2, 1.0))        # (j1, j2, dt / delt): two consecutive leapfrog steps ...
STARTUP = ((1, 1, 0.5), (1, 2, 1.0))         # ... and the start-up pair of first_step (time_stepping.f90:12-24)
TAGS = {8: "t30", 5: "t30k5", 7: "t30k7"}    # kx -> the variant with the reference's own half levels


def plan_of_levels(kx, nmem):
    """the T30 plan of kx levels for nmem members: the reference's own sets (TAGS), any other count on tests/levels.py's half levels"""
    return support.ensemble_plan(TAGS[kx], nmem) if kx in TAGS else levels.plan("t30", kx, nmem * (4 * kx + 4))


def member_states(sp, nmem, seed=8000):
    """nmem single-state dicts with distinct prognostics; phis, tcorh, qcorh (shared by an ensemble) are member 0's in all"""
    sts = [dyn_state(sp, seed + 1000 * e) for e in range(nmem)]
    for st in sts[1:]:
        for n in ("phis", "tcorh", "qcorh"):
            st[n] = sts[0][n]
    return sts


def build(sp, sts):
    import speedy_f90_amd as s
    ens = s.Ensemble(sp, len(sts))
    ens.set_shared(sts[0])
    for e, st in enumerate(sts):
        ens.set_member(e, st)
    return ens


def snapshot(ens):
    """clones of everything a step leaves that the tests compare"""
    return {n: getattr(ens, n).clone() for n in COMPARED}


def member_of(snap, e):
    """member e of an ensemble snapshot in the single state's layout: vor .. tr (2, kx, ..), ps (2, ..), phi (kx, ..), U, V (3 kx, ..),
    PL (3 kx + 1, ..)"""
    E, kx = snap["phi"].shape[:2]
    grid = tuple(snap["U"].shape[-2:])
    out = {n: snap[n][:, e] for n in PROG}
    out["phi"] = snap["phi"][e]
    for n in ("U", "V"):
        out[n] = snap[n][:, e].reshape((3 * kx,) + grid)
    import torch
    lev = snap["PL"][:3 * E * kx].view((3, E, kx) + grid)[:, e].reshape((3 * kx,) + grid)
    out["PL"] = torch.cat([lev, snap["PL"][3 * E * kx + e][None]])
    return out


def single_snapshot(D, W):
    out = {n: D[n].clone() for n in PROG}
    out.update(phi=W.phi.clone(), U=W.U.clone(), V=W.V.clone(), PL=W.PL.clone())
    return out


def run_ensemble(sp, ens, seq, delt, eps=ROB, physics=None):
    """the steps of seq (initialize_implicit before each, as first_step does) on the ensemble; returns the snapshot after each"""
    snaps = []
    for n, (j1, j2, f) in enumerate(seq):
        sp.initialize_implicit(f * delt)
        ens.step(j1, j2, f * delt, None if physics is None else physics(n), eps=eps)
        sp.synchronize()
        snaps.append(snapshot(ens))
    return snaps


def run_single(sp, st, seq, delt, eps=ROB, physics=None):
    """the same steps on one state through the single-state entry points (modelstep.step, the composite form)"""
    D, W = modelstep.device_state(st), modelstep.Workspace(sp)
    snaps = []
    for n, (j1, j2, f) in enumerate(seq):
        sp.initialize_implicit(f * delt)
        modelstep.step(sp, D, W, f * delt, j1, j2, eps, physics=None if physics is None else physics(n))
        sp.synchronize()
        snaps.append(single_snapshot(D, W))
    return snaps


def differing(sp, ens_snaps, e, st, seq, delt, eps=ROB, names=COMPARED):
    """[(step, array)] where member e of the ensemble run is not bit-equal to the single run on its state"""
    bad = []
    for n, (got, want) in enumerate(zip(ens_snaps, run_single(sp, st, seq, delt, eps))):
        m = member_of(got, e)
        bad += [(n, k) for k in names if not support.same_bits(m[k], want[k])]
    return bad


def relerr(a, b):
    a, b = a.cpu().numpy(), b.cpu().numpy()
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def physics_members(sp, o, E, hsg=None, seeds=None):
    """E physically shaped states over member 0's orography, per-member boundary fields; member 0 is physstep's own case.  hsg,
    seeds: the half levels of sp and o and the case's seeds at a count of tests/levels.py"""
    d0, m0, b0 = seeds = physstep.SEEDS["t30"] if seeds is None else seeds
    case = physstep.Case("t30", sp, o, hsg=hsg, seeds=seeds)
    sts, bnds = [case.st], [case.bnd]
    for e in range(1, E):
        st = moist.state(o, dyn_state(sp, d0 + 1000 * e), m0 + 10 * e)
        for n in ("phis", "tcorh", "qcorh"):
            st[n] = case.st[n]
        sts.append(st)
        bnds.append(physstep.draw_boundary(physstep.grids_of(o, st)["tg"][-1].reshape(-1), b0 + 100 * e))
    sp.surface_set_orography(case.phis0)
    return sts, bnds


def ens_physics(sp, bnds):
    """the ensemble's physics dict: every boundary field (E, il, ix), E radiation states back to back"""
    import torch
    dev = [physstep.device_boundary(b, sp.il, sp.ix) for b in bnds]
    bnd = {n: torch.cat([d[n] for d in dev]) for n in dev[0]}
    rad = torch.full((len(bnds) * sp.radiation_state_size(),), float("nan"), dtype=torch.float64, device="cuda")
    return {"bnd": bnd, "albsfc": bnd["albsfc"], "rad": rad}
