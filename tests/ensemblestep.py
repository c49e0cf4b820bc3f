"""What the ensemble tests share: members with DIFFERENT states (distinct seeds of dynstep.state; equal members would prove nothing
about addressing), the ensemble built from them, a member's part of an ensemble snapshot in the single state's layout, and the
single-state run (modelstep.step) that every member is compared with."""
import numpy as np

import modelstep
from dynstep import ROB
from dynstep import state as dyn_state

PROG = ("vor", "div", "t", "tr", "ps")
COMPARED = PROG + ("phi", "U", "V", "PL")
LEAPFROG = ((2, 2, 1.0), (2, 2, 1.0))        # (j1, j2, dt / delt): two consecutive leapfrog steps ...
STARTUP = ((1, 1, 0.5), (1, 2, 1.0))         # ... and the start-up pair of first_step (time_stepping.f90:12-24)


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


def same_bits(a, b):
    """bit for bit, NaN payloads included"""
    import torch
    if a.shape != b.shape:
        return False
    if a.is_complex():
        a, b = torch.view_as_real(a.contiguous()), torch.view_as_real(b.contiguous())
    return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


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
        bad += [(n, k) for k in names if not same_bits(m[k], want[k])]
    return bad


def relerr(a, b):
    a, b = a.cpu().numpy(), b.cpu().numpy()
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))
