"""CPU: the one copy of the model step that the GPU tests and the rate tools share (tests/modelstep.py) -- its call sequence, the
tensors each call is handed and the time levels it reads, recorded from a stand-in for the plan at made-up small dimensions."""
import pytest
import torch

import modelstep
from dynstep import ROB, SDRAG, WIL

KX, NX, MX, IL, IX = 5, 4, 3, 6, 8
P3 = 3 * KX

INVERSE = ["inverse_batch_segs_dev"]
TAIL = {"composite": ["direct_batch_spectral_step_dev"],
        "one_launch": ["direct_batch_dev", "spectral_step_dev"],
        "separate": ["direct_batch_dev", "tendency_combine_dev", "spectral_tendencies_dev", "implicit_terms_dev", "hdiff_step_dev",
                     "step_fields_dev"]}
HEAD = {"composite": INVERSE, "one_launch": INVERSE, "separate": INVERSE + ["grad_to_grid_dev"]}


class Recorder:
    """stands in for the plan (and for the SPPT pattern): every method call is appended to `calls` as (name, args, kwargs)"""
    kx, nx, mx, il, ix = KX, NX, MX, IL, IX

    def __init__(self, calls=None):
        self.calls = [] if calls is None else calls

    def __getattr__(self, name):
        return lambda *a, **k: self.calls.append((name, a, k))

    def names(self):
        return [c[0] for c in self.calls]

    def args(self, name):
        hits = [c for c in self.calls if c[0] == name]
        assert len(hits) == 1, (name, self.names())
        return hits[0][1], hits[0][2]


def same(a, b):
    """the same view of the same memory"""
    return a.data_ptr() == b.data_ptr() and a.shape == b.shape and a.stride() == b.stride() and a.dtype == b.dtype


def all_same(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        if torch.is_tensor(w):
            assert torch.is_tensor(g) and same(g, w), i
        elif isinstance(w, (list, tuple)):
            all_same(g, w)
        else:
            assert g is w or g == w, (i, g, w)


def make():
    sp = Recorder()
    W = modelstep.Workspace(sp, device="cpu")
    c128 = lambda *s: torch.zeros(s, dtype=torch.complex128)
    D = {n: c128(2, KX, NX, MX) for n in ("vor", "div", "t", "tr")}
    D.update(ps=c128(2, NX, MX), phis=c128(NX, MX), tcorh=c128(NX, MX), qcorh=c128(NX, MX))
    f64 = lambda: torch.zeros((1, IL, IX), dtype=torch.float64)
    Pb = {"bnd": {"albsfc": f64(), "sst": f64()}, "rad": torch.zeros(7, dtype=torch.float64)}
    return sp, D, W, Pb


def test_workspace_buffers_and_views():
    """today's 13 shapes and dtypes; every named view is the hand slice the step sites used to write"""
    sp, D, W, _ = make()
    f, c = torch.float64, torch.complex128
    want = {"ug": (KX, f), "vg": (KX, f), "plain_g": (4 * KX, f), "px": (1, f), "py": (1, f), "U": (P3, f), "V": (P3, f),
            "PL": (P3 + 1, f), "pvor": (P3, c), "pdiv": (P3, c), "pspec": (P3 + 1, c), "phi": (KX, c), "phim": (KX, c)}
    for n, (lead, dt) in want.items():
        t = getattr(W, n)
        assert t.dtype == dt and tuple(t.shape) == ((lead, IL, IX) if dt == f else (lead, NX, MX)) and t.is_contiguous(), n
        assert not t.any(), n
    assert len({getattr(W, n).data_ptr() for n in want}) == 13
    g, kx = W.plain_g, KX
    views = {"vorg": g[:kx], "divg": g[kx:2 * kx], "tg": g[2 * kx:3 * kx], "trg": g[3 * kx:],
             "utend": W.U[:kx], "vtend": W.V[:kx], "ttend": W.PL[kx:2 * kx], "qtend": W.PL[2 * kx:3 * kx],
             "vordt": W.pvor[:kx], "divdt": W.pdiv[:kx], "tdt": W.pdiv[kx:2 * kx], "trdt": W.pdiv[2 * kx:], "psdt": W.pspec[3 * kx]}
    for n, v in views.items():
        assert same(getattr(W, n), v), n
    assert tuple(W.trg.shape) == (KX, IL, IX) and tuple(W.trdt.shape) == (KX, NX, MX) and tuple(W.psdt.shape) == (NX, MX)


def expected_head(D, W, lv, form):
    src = [D[n][lv] for n in ("vor", "div", "t", "tr")]
    lead = (D["vor"][lv], D["div"][lv], W.ug, W.vg, src, W.plain_g)
    grad = (D["ps"][lv:lv + 1], W.px, W.py)
    kw = {"kcos_pairs": 2, "kcos": 1}
    if form == "separate":
        return [("inverse_batch_segs_dev", lead, kw), ("grad_to_grid_dev", grad + (2,), {})]
    return [("inverse_batch_segs_dev", lead + grad, kw)]


def expected_tail(D, W, form, j1, dt, eps):
    g, kx = W.plain_g, KX
    prog = (D["vor"], D["div"], D["t"], D["tr"], D["ps"], D["phis"], D["tcorh"], D["qcorh"])
    calls = [("grid_tendencies_dev", (W.ug, W.vg, g[2 * kx:3 * kx], g[:kx], g[kx:2 * kx], g[3 * kx:], W.px, W.py, W.U, W.V, W.PL), {})]
    if form == "composite":
        return calls + [("direct_batch_spectral_step_dev", (W.U, W.V, W.PL, W.pvor, W.pdiv, W.pspec) + prog +
                         (SDRAG, j1, dt, eps, WIL, W.phi), {"kcos": 2})]
    calls.append(("direct_batch_dev", (W.U, W.V, W.pvor, W.pdiv, W.PL, W.pspec), {"kcos": 2}))
    if form == "one_launch":
        return calls + [("spectral_step_dev", (W.pvor, W.pdiv, W.pspec) + prog + (SDRAG, j1, dt, eps, WIL, W.phi), {})]
    vordt, divdt, tdt, trdt, psdt = W.pvor[:kx], W.pdiv[:kx], W.pdiv[kx:2 * kx], W.pdiv[2 * kx:], W.pspec[3 * kx]
    return calls + [
        ("tendency_combine_dev", (W.pdiv, W.pspec), {}),
        ("spectral_tendencies_dev", (D["div"][0], D["t"][0], D["ps"][0], D["phis"], divdt, tdt, psdt, W.phi), {}),
        ("implicit_terms_dev", (divdt, tdt, psdt), {}),
        ("hdiff_step_dev", (D["vor"][0], D["div"][0], D["t"][0], D["tr"][0], D["tcorh"], D["qcorh"], SDRAG, vordt, divdt, tdt, trdt), {}),
        ("step_fields_dev", ([(D["ps"], psdt), (D["vor"], vordt), (D["div"], divdt), (D["t"], tdt), (D["tr"], trdt)], j1, dt, eps, WIL), {})]


def check(calls, want):
    assert [c[0] for c in calls] == [w[0] for w in want]
    for (name, a, k), (_, wa, wk) in zip(calls, want):
        all_same(a, wa)
        assert k == wk, name


@pytest.mark.parametrize("j1,j2,eps", [(2, 2, ROB), (1, 1, 0.0), (1, 2, 0.0)])
@pytest.mark.parametrize("form", modelstep.FORMS)
def test_adiabatic_step(form, j1, j2, eps):
    """every form: the documented sequence, the hand slices as arguments, level j2 - 1 of the prognostics in the inverse batch,
    j1 / dt / eps in the tail"""
    sp, D, W, _ = make()
    modelstep.step(sp, D, W, 1234.5, j1, j2, eps, form=form)
    assert sp.names() == HEAD[form] + ["grid_tendencies_dev"] + TAIL[form]
    check(sp.calls, expected_head(D, W, j2 - 1, form) + expected_tail(D, W, form, j1, 1234.5, eps))
    if j2 == 1:                                        # level 0, and not level 1 of the same array
        a, _ = sp.args("inverse_batch_segs_dev")
        assert a[0].data_ptr() == D["vor"].data_ptr() != D["vor"][1].data_ptr()


def test_defaults_are_the_leapfrog_step():
    sp, D, W, _ = make()
    modelstep.step(sp, D, W, 600.0)
    check(sp.calls, expected_head(D, W, 1, "composite") + expected_tail(D, W, "composite", 2, 600.0, ROB))
    with pytest.raises(AssertionError):
        modelstep.step(sp, D, W, 600.0, form="fused")


def physics_calls(D, W, Pb, kind, sw, pat=None, advance=True, out=None):
    kx = KX
    tend = (W.U[:kx], W.V[:kx], W.PL[kx:2 * kx], W.PL[2 * kx:3 * kx])
    geo = ("geopotential_dev", (D["t"][0], D["phis"], W.phim), {})
    spec = (D["vor"][0], D["div"][0], D["t"][0], D["tr"][0], W.phim, D["ps"][0], Pb["bnd"], Pb["bnd"]["albsfc"], Pb["rad"])
    if kind == "moist":
        return [geo, ("moist_physics_dev", (D["t"][0], D["tr"][0], W.phim, D["ps"][0]) + tend[2:], {})]
    if kind == "whole":
        return [geo, ("physics_dev", (sw,) + spec + tend + (out,), {})]
    return [geo] + ([("advance_dev", (), {})] if advance else []) + [("physics_sppt_dev", (pat, sw) + spec + tend, {})]


@pytest.mark.parametrize("j2", [2, 1])
@pytest.mark.parametrize("kind", ["moist", "whole", "whole_out", "sppt", "sppt_no_advance"])
def test_step_with_physics(kind, j2):
    """the physics sits between the grid tendencies and the direct batch, begins with the geopotential of level 0 and reads level 0
    of D whatever j2 is; SPPT: geopotential, advance, physics_sppt_dev, and without the advance when told so"""
    sp, D, W, Pb = make()
    pat = Recorder(sp.calls)                           # the pattern's advance lands in the same record
    held = {"rad": {"ssrd": torch.zeros(1, IL, IX, dtype=torch.float64)}}
    if kind == "moist":
        phys, want = modelstep.moist_physics(), physics_calls(D, W, Pb, "moist", None)
    elif kind.startswith("whole"):
        out = held if kind == "whole_out" else None
        phys, want = modelstep.whole_physics(Pb, True, out), physics_calls(D, W, Pb, "whole", True, out=out)
    else:
        adv = kind == "sppt"
        phys, want = modelstep.sppt_physics(Pb, False, pat, advance=adv), physics_calls(D, W, Pb, "sppt", False, pat, adv)
    modelstep.step(sp, D, W, 300.0, 1 if j2 == 1 else 2, j2, 0.0 if j2 == 1 else ROB, physics=phys)
    names = {"moist": ["geopotential_dev", "moist_physics_dev"], "whole": ["geopotential_dev", "physics_dev"],
             "whole_out": ["geopotential_dev", "physics_dev"], "sppt": ["geopotential_dev", "advance_dev", "physics_sppt_dev"],
             "sppt_no_advance": ["geopotential_dev", "physics_sppt_dev"]}[kind]
    assert sp.names() == INVERSE + ["grid_tendencies_dev"] + names + TAIL["composite"]
    tail = expected_tail(D, W, "composite", 1 if j2 == 1 else 2, 300.0, 0.0 if j2 == 1 else ROB)
    check(sp.calls, expected_head(D, W, j2 - 1, "composite") + tail[:1] + want + tail[1:])
    a, _ = sp.args("geopotential_dev")                 # level 0 itself: the array's own start
    assert a[0].data_ptr() == D["t"].data_ptr() != D["t"][1].data_ptr()


def test_physics_is_any_callable():
    """physics(sp, D, W) is called once, after the grid tendencies and before the direct batch, in every form"""
    for form in modelstep.FORMS:
        sp, D, W, _ = make()
        seen = []
        modelstep.step(sp, D, W, 300.0, physics=lambda *a: (seen.append(a), sp.mark()), form=form)
        assert len(seen) == 1 and seen[0][0] is sp and seen[0][1] is D and seen[0][2] is W
        assert sp.names() == HEAD[form] + ["grid_tendencies_dev", "mark"] + TAIL[form]


def test_startup():
    """time_stepping.f90:12-24: initialize_implicit(delt / 2), step(1, 1), initialize_implicit(delt), step(1, 2),
    initialize_implicit(2 delt), a synchronize after each step; the steps are numbered -1 and 0"""
    sp = Recorder()
    modelstep.startup(sp, 2400.0, lambda *a: sp.step(*a))
    assert sp.calls == [("initialize_implicit", (1200.0,), {}), ("step", (1, 1, 1200.0, -1), {}), ("synchronize", (), {}),
                        ("initialize_implicit", (2400.0,), {}), ("step", (1, 2, 2400.0, 0), {}), ("synchronize", (), {}),
                        ("initialize_implicit", (4800.0,), {})]
