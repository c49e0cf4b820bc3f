"""GPU: surface fluxes and vertical diffusion on the device (csrc/spdy_surface.hip; physics.f90:169-170, :193-205) -- each kernel
with every optional output against the flang-built reference's fixture and the restatement, batch composition, the whole chain
(spdy_column_physics_dev) on a shortwave step and a step without shortwave against the chain of restatements and the five single
calls, and the chain captured in one graph with a new date and new boundary values between two replays."""
import os

import numpy as np
import pytest

import radiation
import support
import surface
import synth
from conftest import GOLDEN, TOL

pytestmark = pytest.mark.gpu


def _close(got, want, key):
    e = synth.relerr(np.asarray(got), np.asarray(want))
    print("  %-8s %.2e" % (key, e))
    assert e <= TOL, (key, e)
    return e


def _orography(sp, c, il, ix, nb=1):
    """the plan's orography is one (ix, il) field: every state of the batch gets the first state's"""
    ph = c["phis0"].reshape(nb, il * ix)
    ph[:] = ph[0]
    sp.surface_set_orography(ph[0].reshape(il, ix))


def _grids(c, names, nb, il, ix):
    return {n: radiation.grids(c[n], nb, il, ix) for n in names}


def _kx_level(a, kx):
    """level kx of a [nb, kx, il, ix] stack as columns"""
    return np.asarray(a)[:, kx - 1].reshape(-1)


@pytest.mark.parametrize("tag", support.PHYSICS_TAGS)
def test_kernels_vs_reference_and_restatement(tag):
    """surface_columns and pbl_columns with every optional output: the stored sample against the reference, every column
    against the restatement."""
    z = np.load(os.path.join(GOLDEN, "ref_surface.npz"))
    ix, il, kx = support.grid(tag)
    sp, tab, c, zon, sqcoa = surface.case(tag, int(z[tag + "_seed"]))
    sub = z[tag + "_sub"]
    sp.surface_set_orography(c["phis0"].reshape(il, ix))
    r, _ = surface.chain(tab, c, zon, sqcoa)
    G = lambda a: radiation.grids(a, 1, il, ix)[0]
    bnd = {n: G(c[n]) for n in surface.BOUNDARY}
    worst = 0.0
    s = sp.surface_columns(G(c["ug"]), G(c["vg"]), G(c["tg"]), G(c["qg"]), G(c["phig"]), G(c["pslg"]), G(r["ssrd"]),
                           G(r["down"]["slrd"]), bnd)
    for n in surface.SFC_OUT:
        got = s[n].reshape(-1, il * ix).squeeze()
        worst = max(worst, _close(got[..., sub], z["%s_%s" % (tag, n)], n), _close(got, r["sfc"][n], n))
    assert np.array_equal(s["fsfcu"].reshape(-1), s["slru"][2].reshape(-1))
    assert np.array_equal(s["flux3"], np.stack([s[n][2] for n in surface.FLUX3]))
    m, up = r["moist"], r["up"]
    p = sp.pbl_columns(G(c["qg"]), G(c["phig"]), G(c["pslg"]), G(m["se"]), G(m["rh"]), G(m["qsat"]), G(m["icnv"]),
                       np.stack([G(f) for f in r["flux3"]]), G(c["utend"]), G(c["vtend"]), G(up["ttend"]), G(m["qtend"]))
    for n in surface.PBL_OUT:
        got = p[n].reshape(-1, il * ix).squeeze()
        want = r["pbl"][n]
        if n in ("utend", "vtend"):
            assert np.array_equal(got[:kx - 1], np.asarray(c[n])[:kx - 1]), n     # untouched above level kx
            got, want = got[kx - 1], want[kx - 1]
        worst = max(worst, _close(got[..., sub], z["%s_%s" % (tag, n)], n), _close(got, want, n))
    sp.close()
    print("\n[surface kernels %s vs reference and restatement] worst %.1e" % (tag, worst))


def _device_inputs(c, r, nb, kx, il, ix):
    import torch
    d = {n: support.dev(radiation.grids(c[n], nb, il, ix)) for n in ("ug", "vg", "tg", "qg", "phig", "pslg", "utend", "vtend", "ttend",
                                                                     "qtend", "albsfc") + surface.BOUNDARY}
    if r is not None:
        d.update(ssrd=support.dev(radiation.grids(r["ssrd"], nb, il, ix)), slrd=support.dev(radiation.grids(r["down"]["slrd"], nb, il, ix)))
        m = r["moist"]
        d.update({n: support.dev(radiation.grids(m[n], nb, il, ix)) for n in ("se", "rh", "qsat")})
        d["icnv"] = support.dev(radiation.grids(m["icnv"], nb, il, ix).astype(np.int32))
        d["flux3"] = support.dev(np.ascontiguousarray(np.moveaxis(np.stack([radiation.grids(f, nb, il, ix) for f in r["flux3"]]), 0, 1)))
        d["ttend_up"] = support.dev(radiation.grids(r["up"]["ttend"], nb, il, ix))
        d["qtend_m"] = support.dev(radiation.grids(m["qtend"], nb, il, ix))
    return d


def test_batch_composition():
    """A state's output bits do not depend on nb or on its position in the batch (nb = 1 against the same state inside nb = 3)."""
    import torch
    nb = 3
    ix, il, kx = support.grid("t30")
    sp, tab, c, zon, sqcoa = surface.case("t30", 9600, nb)
    _orography(sp, c, il, ix, nb)
    r, _ = surface.chain(tab, c, zon, sqcoa)
    d = _device_inputs(c, r, nb, kx, il, ix)

    def run(D, n):
        o = sp.column_outputs(n, ("sfc", "pbl"))
        o.update(ts=torch.zeros_like(D["pslg"]), fsfcu=torch.zeros_like(D["pslg"]), flux3=torch.zeros_like(D["flux3"]))
        o.update({k: D[s].clone() for k, s in (("U", "utend"), ("V", "vtend"), ("T", "ttend_up"), ("Q", "qtend_m"))})
        sp.surface_fluxes_dev(D["ug"], D["vg"], D["tg"], D["qg"], D["phig"], D["pslg"], D["ssrd"], D["slrd"], D, o["ts"], o["fsfcu"],
                              o["flux3"], o["sfc"])
        sp.pbl_dev(D["qg"], D["phig"], D["pslg"], D["se"], D["rh"], D["qsat"], D["icnv"], D["flux3"], o["U"], o["V"], o["T"], o["Q"],
                   o["pbl"])
        torch.cuda.synchronize()
        return o
    full = run(d, nb)
    for b in range(nb):
        one = run({n: v[b:b + 1].contiguous() for n, v in d.items()}, 1)
        for n in ("ts", "fsfcu", "flux3", "U", "V", "T", "Q"):
            assert torch.equal(one[n][0], full[n][b]), (b, n)
        for grp in ("sfc", "pbl"):
            for n in one[grp]:
                assert torch.equal(one[grp][n][0], full[grp][n][b]), (b, n)
    sp.close()


def _second_step(c, tab, kx):
    """the inputs of the step without shortwave: radiation.py's second temperatures, new winds and boundary values"""
    c2 = dict(c)
    c2.update(tg=c["tg2"], ug=c["vg"], vg=c["ug"], sst=c["sst"] + 0.5, stl=c["stl"] - 0.5, ttend=c["ttend2"])
    return c2


@pytest.mark.parametrize("tag", ["t30", "t63k16"])
def test_column_physics_chain_and_capture(tag):
    """spdy_column_physics_dev on a shortwave step and then a step without shortwave on the held radiation state: within TOL of
    the chain of restatements and bit-equal to the five single device calls; the two steps captured in one graph and replayed
    twice with a new date and new boundary values between the replays are bit-equal to plain launches, and the graph has the
    moist + radiation node count plus 2 per step."""
    import torch
    nb = 2
    ix, il, kx = support.grid(tag)
    sp, tab, c, zon, sqcoa = surface.case(tag, 9700, nb)
    _orography(sp, c, il, ix, nb)
    c2 = _second_step(c, tab, kx)
    d1, d2 = _device_inputs(c, None, nb, kx, il, ix), _device_inputs(c2, None, nb, kx, il, ix)
    S = sp.radiation_state_size()
    sp.column_physics_workspace()

    def fresh():
        D = {"st": torch.full((nb * S,), float("nan"), dtype=torch.float64, device="cuda")}
        for i, d in ((1, d1), (2, d2)):
            D["t%d" % i] = [d[n].clone() for n in ("utend", "vtend", "ttend", "qtend")]
            D["o%d" % i] = sp.column_outputs(nb, names=surface.SFC_OUT + surface.PBL_OUT + ("slrd", "olr", "icnv", "precnv"))
        return D

    def chain(D):
        for i, d, sw in ((1, d1, True), (2, d2, False)):
            sp.column_physics_dev(sw, d["ug"], d["vg"], d["tg"], d["qg"], d["phig"], d["pslg"], d, d["albsfc"], D["st"], *D["t%d" % i],
                                  D["o%d" % i])

    def flat(D):
        out = {"st": D["st"]}
        for i in (1, 2):
            out.update({"%s%d" % (n, i): v for n, v in zip("UVTQ", D["t%d" % i])})
            o = D["o%d" % i]
            out.update({"%s%d" % (n, i): v for g in ("sfc", "pbl", "rad", "moist") for n, v in o[g].items()})
            out.update({"ts%d" % i: o["ts"], "fsfcu%d" % i: o["fsfcu"]})
        return out

    P = fresh()
    chain(P)
    torch.cuda.synchronize()
    # the chain of restatements, both steps
    r1, st = surface.chain(tab, c, zon, sqcoa, True)
    r2, _ = surface.chain(tab, c2, zon, sqcoa, False, st)
    worst = 0.0
    for i, r in ((1, r1), (2, r2)):
        o, t = P["o%d" % i], P["t%d" % i]
        got = lambda x: radiation.cols(x.cpu().numpy())
        for n, v in zip(("utend", "vtend"), t[:2]):
            worst = max(worst, _close(_kx_level(v.cpu().numpy(), kx), r["pbl"][n][kx - 1], n))
        for n, v in zip(("ttend", "qtend"), t[2:]):
            worst = max(worst, _close(got(v), r["pbl"][n], n))
        for n in ("tt_pbl", "qt_pbl"):
            worst = max(worst, _close(got(o["pbl"][n]), r["pbl"][n], n))
        for n in surface.SFC_3 + ("hfluxn",):
            worst = max(worst, _close(np.moveaxis(o["sfc"][n].cpu().numpy(), 1, 0).reshape(-1, nb * il * ix), r["sfc"][n], n))
        for n in ("tskin", "u0", "v0", "t0"):
            worst = max(worst, _close(got(o["sfc"][n]), r["sfc"][n], n))
        worst = max(worst, _close(got(o["ts"]), r["sfc"]["ts"], "ts"), _close(got(o["fsfcu"]), r["sfc"]["slru"][2], "fsfcu"))
        worst = max(worst, _close(got(o["rad"]["slrd"]), r["down"]["slrd"], "slrd"), _close(got(o["rad"]["olr"]), r["up"]["olr"], "olr"))
        assert np.array_equal(got(o["moist"]["icnv"]), r["moist"]["icnv"])
    print("\n[column physics %s, two steps, vs the chain of restatements] worst %.1e" % (tag, worst))

    # the five single device calls: bit-equal
    Q = fresh()
    mo = sp.column_outputs(nb, "moist", names=("se", "rh", "qsat", "precnv", "precls", "iptop", "icnv"))
    ssrd = torch.zeros_like(d1["pslg"])
    for i, d, sw in ((1, d1, True), (2, d2, False)):
        U, V, T, Qt = Q["t%d" % i]
        o = Q["o%d" % i]
        ro = dict(o["rad"], ssrd=ssrd) if sw else dict(o["rad"])
        flux3 = torch.zeros((nb, 4, il, ix), dtype=torch.float64, device="cuda")
        sp.moist_columns_dev(d["tg"], d["qg"], d["phig"], d["pslg"], T, Qt, mo)
        sp.radiation_down_dev(sw, d["tg"], d["qg"], d["phig"], d["pslg"], mo["rh"], mo["precnv"], mo["precls"], mo["iptop"],
                              d["fmask"], d["albsfc"], Q["st"], ro)
        sp.surface_fluxes_dev(d["ug"], d["vg"], d["tg"], d["qg"], d["phig"], d["pslg"], ssrd, ro["slrd"], d, o["ts"], o["fsfcu"],
                              flux3, o["sfc"])
        sp.radiation_up_dev(d["tg"], d["pslg"], o["ts"], o["fsfcu"], Q["st"], T, ro)
        sp.pbl_dev(d["qg"], d["phig"], d["pslg"], mo["se"], mo["rh"], mo["qsat"], mo["icnv"], flux3, U, V, T, Qt, o["pbl"])
        o["moist"]["icnv"].copy_(mo["icnv"])
        o["moist"]["precnv"].copy_(mo["precnv"])
    torch.cuda.synchronize()
    fp, fq = flat(P), flat(Q)
    for n in fp:
        assert torch.equal(fp[n], fq[n]), ("single calls", n)

    # node counts: the chain has the moist + radiation launches plus 2
    with sp.graph_capture() as g0:
        for i, d, sw in ((1, d1, True), (2, d2, False)):
            T, Qt = Q["t%d" % i][2:]
            sp.moist_columns_dev(d["tg"], d["qg"], d["phig"], d["pslg"], T, Qt, mo)
            sp.radiation_down_dev(sw, d["tg"], d["qg"], d["phig"], d["pslg"], mo["rh"], mo["precnv"], mo["precls"], mo["iptop"],
                                  d["fmask"], d["albsfc"], Q["st"], None)
            sp.radiation_up_dev(d["tg"], d["pslg"], Q["o1"]["ts"], Q["o1"]["fsfcu"], Q["st"], T, None)
    base_nodes = g0.num_nodes()
    g0.close()
    D = fresh()
    torch.cuda.synchronize()
    with sp.graph_capture() as g:
        chain(D)
    assert g.num_nodes() == base_nodes + 2 * 2, (g.num_nodes(), base_nodes)
    g.launch()
    sp.synchronize()
    fd = flat(D)
    for n in fp:
        assert torch.equal(fd[n], fp[n]), ("captured", n)
    # a new date and new boundary values between two replays: bit-equal to plain launches on the same values
    sp.radiation_set_date(radiation.DATES[1])
    for d in (d1, d2):
        d["sst"].add_(1.25)
        d["soilw"].mul_(0.5)
        d["alb_l"].mul_(0.9)
    F = fresh()
    for n, v in flat(F).items():
        fd[n].copy_(v)
    torch.cuda.synchronize()
    g.launch()
    sp.synchronize()
    chain(F)
    torch.cuda.synchronize()
    ff = flat(F)
    changed = 0
    for n in fp:
        assert torch.equal(fd[n], ff[n]), ("replayed", n)
        changed += int(not torch.equal(fd[n], fp[n]))
    assert changed > 10                                   # the replay followed the new date and boundary values
    g.close()
    sp.close()


def test_state_errors_on_device():
    """SPDY_ERR_STATE without the orography on a device plan; the boundary layer needs none."""
    import speedy_f90_amd as s
    ix, il, kx = support.grid("t30")
    sp = support.plan("t30", 4)
    import torch
    g3, g2, g4 = (torch.zeros((1,) + lead + (il, ix), dtype=torch.float64, device="cuda") for lead in ((kx,), (), (4,)))
    bnd = {n: g2 for n in surface.BOUNDARY}
    with pytest.raises(s.SpdyError) as e:
        sp.surface_fluxes_dev(g3, g3, g3, g3, g3, g2, g2, g2, bnd, g2.clone(), g2.clone(), g4)
    assert e.value.code == -5
    sp.close()


def test_column_physics_numpy_form_equals_device_form():
    """column_physics (the NumPy form of the chain) on a shortwave step, then without shortwave on the returned state, at the
    smallest grid and level count: the returned keys are the documented ones (no shortwave-only key on the second call) and every
    returned array is bit-equal to the tensor column_physics_dev leaves in column_outputs buffers given the same inputs -- the
    same kernels on the same bytes."""
    import torch
    nb, tag = 2, "t30k5"
    ix, il, kx = support.grid(tag)
    sp, tab, c, zon, sqcoa = surface.case(tag, 9800, nb)
    _orography(sp, c, il, ix, nb)
    tend, sw_only = ("utend", "vtend", "ttend", "qtend"), {"cloudc", "clstr", "icltop", "ssr", "tsr", "tt_rsw"}
    always = set(tend + ("state", "ts", "fsfcu", "precnv", "precls", "cbmf", "iptop", "icnv", "qsat", "rh", "se", "slrd", "slr", "olr",
                         "tt_rlw", "ut_pbl", "vt_pbl", "tt_pbl", "qt_pbl") + surface.SFC_OUT)       # rad.ssrd stays in the plan's workspace
    out = sp.column_outputs(nb)            # one set for both steps: the caller's rad.ssrd is read by the step without shortwave
    by_name = {n: t for b in ("moist", "rad", "sfc", "pbl") for n, t in out[b].items()}
    by_name.update(ts=out["ts"], fsfcu=out["fsfcu"])
    by_name["state"] = torch.zeros(nb * sp.radiation_state_size(), dtype=torch.float64, device="cuda")
    state = None
    for cols, sw in ((c, True), (_second_step(c, tab, kx), False)):
        g = {n: radiation.grids(cols[n], nb, il, ix) for n in ("ug", "vg", "tg", "qg", "phig", "pslg", "albsfc") + tend + surface.BOUNDARY}
        res = sp.column_physics(*[g[n] for n in ("ug", "vg", "tg", "qg", "phig", "pslg")], {n: g[n] for n in surface.BOUNDARY},
                                g["albsfc"] if sw else None, *[g[n] for n in tend], compute_sw=sw, state=state)
        state = res["state"]
        assert set(res) == always | (sw_only if sw else set()), sorted(set(res) ^ always)
        d = {n: support.dev(a) for n, a in g.items()}
        sp.column_physics_dev(sw, d["ug"], d["vg"], d["tg"], d["qg"], d["phig"], d["pslg"], d, d["albsfc"] if sw else None,
                              by_name["state"], *[d[n] for n in tend], out)
        torch.cuda.synchronize()
        for n, a in res.items():
            want = (d[n] if n in tend else by_name[n]).cpu().numpy()
            assert a.dtype == want.dtype and np.array_equal(a, want), (sw, n)
    sp.close()
