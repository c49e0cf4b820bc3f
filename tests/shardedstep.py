"""The level-sharded time step with ranks inside one process: what tests/test_gpu_sharded_step.py and tests/test_gpu_levels.py share --
the plan and oracle of a variant or of a (resolution, kx) pair of tests/levels.py, the unsharded device step both forms are held to,
the thread one rank runs in, and the two checks (the all-gather form, the transposed form) on a tag and a rank count."""
import threading

import numpy as np

import levels
import modelstep
import synth
from conftest import TOL, VARIANTS
from dynstep import ROB, SDRAG, WIL, oracle_dynamics_step, state, wave_relerr

DT = 2400.0
PROGS = ("vor", "div", "t", "tr", "ps")


def level_count(tag):
    """tag: a key of conftest.VARIANTS, or a (trunc_tag, kx) pair of tests/levels.py"""
    return tag[1] if isinstance(tag, tuple) else VARIANTS[tag][3]


def is_t30(tag):
    return (tag[0] if isinstance(tag, tuple) else tag).startswith("t30")


def oracle_of(tag, oracle_factory):
    return levels.oracle(*tag) if isinstance(tag, tuple) else oracle_factory(tag)


def make_plan(tag, device=0):
    import speedy_f90_amd as s
    if isinstance(tag, tuple):
        sp = levels.plan(tag[0], tag[1], 4 * tag[1] + 4, device)
        sp.initialize_implicit(DT)
        return sp
    trunc, ix, iy, kx = VARIANTS[tag]
    sp = s.Spectral((trunc, ix, iy), kx=kx, max_batch=4 * kx + 4, device=device)
    if tag in synth.SIGMA_SETS:
        sp.set_sigma(synth.SIGMA_SETS[tag])
    sp.initialize_implicit(DT)
    return sp


def unsharded_device_steps(sp, st, nsteps):
    """The three-call device step (tests/modelstep.py) on one plan: prognostics, tendencies and direct-batch operands."""
    import torch
    kx = sp.kx
    D, W = modelstep.device_state(st), modelstep.Workspace(sp)
    for _ in range(nsteps):
        modelstep.step(sp, D, W, DT)
    torch.cuda.synchronize()
    out = {n: D[n].cpu().numpy() for n in PROGS}
    out["phi"] = W.phi.cpu().numpy()
    out["tend"] = np.concatenate([W.pvor[:kx].cpu().numpy(), W.pdiv.cpu().numpy(), W.pspec[3 * kx:].cpu().numpy()])   # vordt | divdt | tdt | trdt | psdt
    out["U"], out["V"], out["PL"] = W.U.cpu().numpy(), W.V.cpu().numpy(), W.PL.cpu().numpy()
    return out


def rank_thread(rank, group, tag, st, nsteps, results, errors, device=0, transpose=False):
    import torch
    import speedy_f90_amd as s
    try:
        torch.cuda.set_device(device)          # (per thread: the tensors below live on the rank's device)
        sp = make_plan(tag, device)
        sp.use_own_stream()
        comm = s.sharding.LevelComm(sp, group=group, rank=rank)
        if transpose:
            comm.set_option("transpose", 1)
        comm.sharded_step_workspace()
        kx, nx, mx = sp.kx, sp.nx, sp.mx
        D = {n: torch.from_numpy(np.ascontiguousarray(st[n])).cuda() for n in st}
        phi = torch.zeros((kx, nx, mx), dtype=torch.complex128, device="cuda")
        tend = torch.zeros((4 * kx + 1, nx, mx), dtype=torch.complex128, device="cuda")
        G, T = comm.sharded_step_stacks()
        torch.cuda.synchronize()
        for step in range(nsteps):
            G.fill_(float("nan")); T.fill_(float("nan"))          # whatever a rank does not compute must ARRIVE, or it poisons the step
            torch.cuda.synchronize()
            if step == 0:                                         # the one call ...
                comm.sharded_step_(D["vor"], D["div"], D["t"], D["tr"], D["ps"], D["phis"], D["tcorh"], D["qcorh"], SDRAG, 2, 2, DT, ROB, WIL,
                                   phi, tend)
            else:                                                 # ... and its two halves (the physics hook sits between them)
                comm.sharded_step_grid_(D["vor"], D["div"], D["t"], D["tr"], D["ps"], 2)
                comm.sharded_step_spectral_(D["vor"], D["div"], D["t"], D["tr"], D["ps"], D["phis"], D["tcorh"], D["qcorh"], SDRAG, 2, DT, ROB,
                                            WIL, phi, tend)
            sp.synchronize()
        U, V, PL, lo, hi = comm.sharded_step_operands()
        out = {}
        if transpose:
            # what the rank holds BEFORE the gather: its coefficient range of every level is current (both time levels)
            desc = comm.describe()
            e0, e1 = desc["coefficients"]
            out["own_range"] = (e0, e1)
            out["before"] = {n: D[n].reshape(D[n].shape[:-2] + (-1,))[..., e0:e1].cpu().numpy() for n in PROGS}
            out["describe"] = desc
            comm.state_gather_(D["vor"], D["div"], D["t"], D["tr"], D["ps"])
            comm.gather_ranges_(phi, tend)
            sp.synchronize()
        out.update({n: D[n].cpu().numpy() for n in PROGS})
        out.update(phi=phi.cpu().numpy(), tend=tend.cpu().numpy(), U=U.cpu().numpy(), V=V.cpu().numpy(), PL=PL.cpu().numpy(), lo=lo, hi=hi)
        results[rank] = out
        comm.close(); sp.close()
    except Exception as e:          # a missing rank would leave the others waiting for the group's timeout
        errors[rank] = e


def in_process_ranks(tag, world, oracle_factory, monkeypatch):
    """the all-gather form on `world` in-process ranks, two steps: against the oracle's call-by-call step within TOL and bit for bit
    against the unsharded device step"""
    import speedy_f90_amd as s
    monkeypatch.setenv("SPDY_COMM_TIMEOUT_S", "60")
    kx = level_count(tag)
    o = oracle_of(tag, oracle_factory)
    o.tail_init(DT)
    sp0 = make_plan(tag)
    st = state(sp0, 8000)
    nsteps = 2
    whole = unsharded_device_steps(sp0, st, nsteps)
    group = s.sharding.LocalGroup(sp0.lib, world)
    results, errors = {}, {}
    threads = [threading.Thread(target=rank_thread, args=(r, group, tag, st, nsteps, results, errors)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(600)
    assert not errors, errors
    assert sorted(results) == list(range(world)), "ranks that returned %s, expected 0..%d" % (sorted(results), world - 1)
    group.close(); sp0.close()
    ref = st
    for _ in range(nsteps):
        ref, out = oracle_dynamics_step(o, ref, 2, DT, ROB)
    ref_tend = np.concatenate([out["vordt"], out["divdt"], out["tdt"], out["trdt"], out["psdt"][None]])
    worst = 0.0
    for r in range(world):
        got = results[r]
        assert (got["lo"], got["hi"]) == s.sharding.shard_range(kx, r, world), (
            "levels of rank %d" % r, got["lo"], got["hi"], s.sharding.shard_range(kx, r, world))
        own = [g * kx + k for g in range(3) for k in range(got["lo"], got["hi"])]
        # vs the oracle's call-by-call step: the north star's bar
        for n in PROGS:
            worst = max(worst, synth.relerr(got[n], ref[n]), wave_relerr(got[n], ref[n]))
        worst = max(worst, wave_relerr(got["phi"], out["phi"]))
        for a in range(4):
            worst = max(worst, wave_relerr(got["tend"][a * kx:(a + 1) * kx], ref_tend[a * kx:(a + 1) * kx]))
        worst = max(worst, synth.relerr(got["tend"][4 * kx], ref_tend[4 * kx]))
        worst = max(worst, synth.relerr(got["U"], out["U"][own]), synth.relerr(got["V"], out["V"][own]),
                    synth.relerr(got["PL"], np.concatenate([out["PL"][own], out["PL"][3 * kx:]])))
        # vs the unsharded device step: same bits, whatever the rank count
        for n in PROGS + ("phi", "tend"):
            assert np.array_equal(got[n], whole[n]), (tag, world, r, n, synth.relerr(got[n], whole[n]))
        assert np.array_equal(got["U"], whole["U"][own]) and np.array_equal(got["V"], whole["V"][own]), (tag, world, r, "U, V against the unsharded step")
        assert np.array_equal(got["PL"], np.concatenate([whole["PL"][own], whole["PL"][3 * kx:]])), (tag, world, r, "PL against the unsharded step")
    print("\n[sharded step %s, %d in-process ranks] worst relative error vs the oracle %.1e; bits equal to the unsharded device step"
          % (tag, world, worst))
    assert worst <= TOL, (tag, world, worst)


def transposed_in_process_ranks(tag, world, oracle_factory, monkeypatch, pays=0.6):
    """the transposed form on `world` in-process ranks (tests/test_gpu_sharded_step.py says what it is).  pays: from four ranks on every
    rank of the transposed form receives less than this part of the all-gather form's bytes (0.6 for the equal level blocks of
    that test's cases)"""
    import speedy_f90_amd as s
    monkeypatch.setenv("SPDY_COMM_TIMEOUT_S", "60")
    kx = level_count(tag)
    o = oracle_of(tag, oracle_factory)
    o.tail_init(DT)
    sp0 = make_plan(tag)
    st = state(sp0, 8000)
    nsteps = 2
    whole = unsharded_device_steps(sp0, st, nsteps)
    group = s.sharding.LocalGroup(sp0.lib, world)
    results, errors = {}, {}
    threads = [threading.Thread(target=rank_thread, args=(r, group, tag, st, nsteps, results, errors, 0, True)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(600)
    assert not errors, errors
    assert sorted(results) == list(range(world)), "ranks that returned %s, expected 0..%d" % (sorted(results), world - 1)
    group.close(); sp0.close()
    ref = st
    for _ in range(nsteps):
        ref, out = oracle_dynamics_step(o, ref, 2, DT, ROB)
    ref_tend = np.concatenate([out["vordt"], out["divdt"], out["tdt"], out["trdt"], out["psdt"][None]])
    exact = is_t30(tag)
    worst, covered = 0.0, 0
    for r in range(world):
        got = results[r]
        own = [g * kx + k for g in range(3) for k in range(got["lo"], got["hi"])]
        for n in PROGS:
            worst = max(worst, synth.relerr(got[n], ref[n]), wave_relerr(got[n], ref[n]))
        worst = max(worst, wave_relerr(got["phi"], out["phi"]))
        for a in range(4):
            worst = max(worst, wave_relerr(got["tend"][a * kx:(a + 1) * kx], ref_tend[a * kx:(a + 1) * kx]))
        worst = max(worst, synth.relerr(got["tend"][4 * kx], ref_tend[4 * kx]))
        worst = max(worst, synth.relerr(got["U"], out["U"][own]), synth.relerr(got["V"], out["V"][own]),
                    synth.relerr(got["PL"], np.concatenate([out["PL"][own], out["PL"][3 * kx:]])))
        # the ranks' coefficient ranges tile the spectrum, and each rank's range was current before the gather
        e0, e1 = got["own_range"]
        covered += e1 - e0
        for n in PROGS:
            flat = whole[n].reshape(whole[n].shape[:-2] + (-1,))[..., e0:e1]
            if exact:
                assert np.array_equal(got["before"][n], flat), (tag, world, r, n)
            else:
                assert synth.relerr(got["before"][n], flat) <= 1e-13, (tag, world, r, n)
        for n in PROGS + ("phi", "tend"):
            if exact:
                assert np.array_equal(got[n], whole[n]), (tag, world, r, n, synth.relerr(got[n], whole[n]))
            else:
                assert synth.relerr(got[n], whole[n]) <= 1e-13, (tag, world, r, n, synth.relerr(got[n], whole[n]))
        # the direct-batch operands of the rank's levels came home complete (exchange 2)
        wpl = np.concatenate([whole["PL"][own], whole["PL"][3 * kx:]])
        if exact:
            assert np.array_equal(got["U"], whole["U"][own]) and np.array_equal(got["V"], whole["V"][own]) and np.array_equal(got["PL"], wpl), (
                tag, world, r, "U, V, PL against the unsharded step")
        else:   # (second step: its inputs already differ by the first step's rounding)
            worst_op = max(synth.relerr(got["U"], whole["U"][own]), synth.relerr(got["V"], whole["V"][own]), synth.relerr(got["PL"], wpl))
            assert worst_op <= 1e-13, (tag, world, r, "U, V, PL against the unsharded step", worst_op)
        d = got["describe"]
        assert d["form"] == "transpose" and d["nranks"] == world and d["rank"] == r, ("describe() of rank %d of %d" % (r, world), d)
        if world >= 4:      # (at two ranks the four exchanges move about what the two all-gathers do; the form pays from four ranks on)
            assert d["bytes_received_per_step_transposed_form"] < pays * d["bytes_received_per_step_allgather_form"], d
    assert covered == results[0]["vor"].shape[-1] * results[0]["vor"].shape[-2], "the ranks' coefficient ranges cover %d of the spectrum's entries" % covered
    print("\n[transposed sharded step %s, %d in-process ranks] worst relative error vs the oracle %.1e; %s the unsharded device step"
          % (tag, world, worst, "bits equal to" if exact else "within 1e-13 of"))
    assert worst <= TOL, (tag, world, worst)
