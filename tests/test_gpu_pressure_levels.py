"""GPU: the pressure-level output (include/spdy.h "pressure-level output", Ensemble.output_pressure) -- every member's
fields on caller-given pressure levels, and the mean and the spread of the interpolated values.

On grids (spdy_ens_output_pressure_grid_dev) the inputs are the test's own (tests/pressurelevels.py: craft), so the statements are
exact: what must be bit-equal is compared bit for bit, everything else against the NumPy restatement within one float32 ulp of the
reference value -- device and restatement differ in exp alone (linear mode; an ulp of FP64, which can move a float32 rounding and
nothing more; the log-p coordinate has no device transcendental at all).  No point is left out of any comparison.
From spectra (Ensemble.output_pressure) the reference is the restatement on the oracle's FP64 grids, and the reference's own route:
np.interp on the float32 snapshot, as scripts/sigma_to_pressure.py does it."""
import numpy as np
import pytest

import ensembleoutput as eo
import ensemblestep as es
import pressurelevels as pl
import support

pytestmark = pytest.mark.gpu

GROUPS = ("members", "mean", "spread")
FIELDS = eo.FIELDS


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ------------------------------------------------------------------------------------------------ on grids
@pytest.fixture(scope="module")
def plans():
    def make(kx):
        import speedy_f90_amd as s
        sp = s.Spectral("t30", kx=kx, max_batch=4 * kx + 4, device=0)
        if kx == 2:
            sp.set_sigma(pl.SIGMA_L2)
        return sp
    with support.plan_cache(make) as get:
        yield get


def run_grid(sp, raw, plev, coord, use=None, groups=GROUPS, below=True):
    """spdy_ens_output_pressure_grid_dev on a crafted ensemble -> {group: {field: array}, "below": array}"""
    import torch
    E, nlev, g = raw["ps"].shape[0], len(plev), (sp.il, sp.ix)
    new = lambda *lead: torch.full(lead + g, -7.0, dtype=torch.float32, device="cuda")
    out = {"members": dict({n: new(E, nlev) for n in pl.QUANTITIES}, ps=new(E)), "mean": dict({n: new(nlev) for n in pl.QUANTITIES}, ps=new()),
           "spread": dict({n: new(nlev) for n in pl.QUANTITIES}, ps=new())}
    out = {grp: d for grp, d in out.items() if grp in groups}
    cnt = new(nlev) if below else None
    if use is not None:
        use = torch.tensor([1 if u else 0 for u in use], dtype=torch.int32, device="cuda")
    sp.ens_output_pressure_grid_dev(E, support.dev(pl.stack(raw)), plev, coord, out.get("members"), out.get("mean"), out.get("spread"), cnt,
                                    use)
    torch.cuda.synchronize()
    res = eo.host(out)
    if below:
        res["below"] = cnt.cpu().numpy()
    return res


def compare(label, got, ref, groups=GROUPS, fields=FIELDS):
    """statement 2: every field of every group within one float32 ulp of the restatement -> the largest error / bound"""
    worst = 0.0
    for grp in groups:
        for n in fields:
            assert got[grp][n].dtype == np.float32 and got[grp][n].shape == ref[grp][n].shape, (grp, n)
            ratio = pl.ulp_excess(got[grp][n], ref[grp][n])
            worst = max(worst, ratio)
            assert ratio <= 1.0, (label, grp, n, ratio)
    print("[plev %s] largest error / (one float32 ulp of the reference): %.3g" % (label, worst))
    return worst


@pytest.mark.parametrize("E", [1, 2, 3, 9, 32])
@pytest.mark.parametrize("nlev", [1, 3, 8])
@pytest.mark.parametrize("kx", [2, 5, 8])
def test_grid_against_restatement(kx, nlev, E, plans):
    """statements 1 and 2 in both coordinates: the classes the inputs hold; a quantity constant in the vertical, a clamped level and a
    target on a level give the bits of (float)x_e[k]; E = 1 gives the member's bits as the mean and spread +0; `below` is the
    restatement's count; every member, mean and spread within one float32 ulp of the restatement"""
    sp = plans(kx)
    fsg = sp.table("fsg")
    raw = pl.craft(sp.ix, sp.il, kx, E, 100 * kx + E)
    xe, plev = pl.values(raw), pl.levels(fsg, nlev)
    for coord in pl.COORDS:
        label = "grid kx=%d nlev=%d E=%d %s" % (kx, nlev, E, coord)
        ref = pl.restate(fsg, xe, raw["ps"], plev, coord)
        cls = ref["cls"]
        found = pl.classes(cls, E)
        if nlev == 8 and E >= 2:
            assert found == pl.every_class(kx, E), (label, sorted(found ^ pl.every_class(kx, E)))
        else:                                                       # fewer levels or one member: what they can hold
            assert "below0" in found and ("on_level" in found) == (kx > 2), (label, sorted(found))
        got = run_grid(sp, raw, plev, coord)
        # 1. bit-exact
        lo, hi, inside = cls["lo"], cls["hi"] & ~cls["lo"], ~cls["lo"] & ~cls["hi"]
        on = inside & (cls["w"] == 0.0)
        for n in pl.QUANTITIES:
            mine, x32 = bits(got["members"][n]), xe[n].astype(np.float32)
            level = lambda k: np.broadcast_to(bits(np.take_along_axis(x32, k, axis=1)), mine.shape)
            first, last, at_kb = level(np.zeros_like(cls["kb"])), level(np.full_like(cls["kb"], kx - 1)), level(cls["kb"])
            assert np.array_equal(mine[lo], first[lo]) and np.array_equal(mine[hi], last[hi]), (label, n)
            assert np.array_equal(mine[on], at_kb[on]), (label, n)
        assert np.array_equal(bits(got["members"]["v"]), np.broadcast_to(bits(raw["v"][:, :1]), (E, nlev, sp.il, sp.ix))), label
        if E == 1:
            for n in FIELDS:
                assert support.same_bits(got["mean"][n], got["members"][n][0]) and not bits(got["spread"][n]).any(), (label, n)
        assert np.array_equal(got["below"], ref["below"].astype(np.float32)), label
        # 2. everything within one float32 ulp
        compare(label, got, ref)


def poisoned(raw):
    """raw with member 1 as tests/test_gpu_isolation.py poisons a member: every field NaN, ps +inf"""
    bad = {n: np.array(a, copy=True) for n, a in raw.items()}
    for n in pl.QUANTITIES:
        bad[n][1] = np.nan
    bad["ps"][1] = np.inf
    return bad


@pytest.mark.parametrize("coord", pl.COORDS)
def test_grid_mask_and_isolation(coord, plans):
    """statement 3: kx = 5, E = 3, member 1 NaN with ps +inf.  Members 0 and 2 keep the clean run's bits and member 1 is NaN on every
    level; with member 1 masked, mean, spread and `below` are bit-equal to the E = 2 ensemble of members 0 and 2; unmasked, mean and
    spread are NaN (member 1 enters everywhere), and `below` -- a count that +inf never joins -- is that of members 0 and 2"""
    sp = plans(5)
    fsg = sp.table("fsg")
    raw = pl.craft(sp.ix, sp.il, 5, 3, 77)
    plev = pl.levels(fsg, 8)
    clean = run_grid(sp, raw, plev, coord)
    bad = poisoned(raw)
    masked, unmasked = run_grid(sp, bad, plev, coord, use=[1, 0, 1]), run_grid(sp, bad, plev, coord)
    pair = run_grid(sp, {n: a[[0, 2]] for n, a in raw.items()}, plev, coord)
    for n in FIELDS:
        for got in (masked, unmasked):
            for e in (0, 2):
                assert support.same_bits(got["members"][n][e], clean["members"][n][e]), (n, e)
            if n != "ps":
                assert np.isnan(got["members"][n][1]).all(), n
        for grp in ("mean", "spread"):
            assert support.same_bits(masked[grp][n], pair[grp][n]) and np.isfinite(masked[grp][n]).all(), (grp, n)
            if n != "ps":
                assert np.isnan(unmasked[grp][n]).all(), (grp, n)
    assert support.same_bits(masked["below"], pair["below"]) and support.same_bits(unmasked["below"], pair["below"])
    assert 0 < pair["below"].max() <= 2
    # on clean members: one in use gives its own values and spread +0, none in use NaN and a count of 0
    one, none = run_grid(sp, raw, plev, coord, use=[0, 1, 0]), run_grid(sp, raw, plev, coord, use=[0, 0, 0])
    for n in FIELDS:
        assert support.same_bits(one["mean"][n], clean["members"][n][1]) and not bits(one["spread"][n]).any(), n
        assert np.isnan(none["mean"][n]).all() and np.isnan(none["spread"][n]).all(), n
        assert support.same_bits(none["members"][n], clean["members"][n]), n
    assert not none["below"].any()
    # the restatement agrees with what a mask means
    ref = pl.restate(fsg, pl.values(bad), bad["ps"], plev, coord, use=[1, 0, 1])
    compare("grid mask %s" % coord, masked, ref, groups=("mean", "spread"))
    assert np.array_equal(masked["below"], ref["below"].astype(np.float32))


@pytest.mark.parametrize("coord", pl.COORDS)
def test_grid_cancellation(coord, plans):
    """statement 4: kx = 8, E = 3, t = 288 + profile[k] + 1e-6 r_e with r_e standard-normal per point and constant in the vertical,
    one surface pressure for all members -- on a pressure level a spread near 1e-6 on values near 288.  The spread of t meets
    statement 2's bound; the one-pass sum of squares, evaluated in FP64 on the restatement's own y_e, does not.
    (The weights are those of the restatement bit for bit here: log-p has no device transcendental, and the linear case sets ps = 0,
    where exp is exact.  An ulp of FP64 in a weight moves y_e by an ulp of 288, 5.7e-14: up to a float32 ulp of a 1e-6 spread.
    The fields on pressure levels are compared; the surface pressure, equal in all members here, has a spread that is the rounding
    residue of sum / 3 on either side, and its fields are held to Ensemble.output's bits in the tests from spectra.)"""
    sp = plans(8)
    fsg = sp.table("fsg")
    r = np.random.default_rng(31)
    raw = pl.craft(sp.ix, sp.il, 8, 3, 78)
    profile = np.linspace(-60.0, 0.0, 8).reshape(1, 8, 1, 1)
    raw["t"] = 288.0 + profile + 1e-6 * r.standard_normal((3, 1, sp.il, sp.ix))
    raw["ps"][:] = 0.0 if coord == "p" else raw["ps"][:1]
    plev = pl.levels(fsg, 8)
    ref = pl.restate(fsg, pl.values(raw), raw["ps"], plev, coord)
    got = run_grid(sp, raw, plev, coord)
    spread = ref["spread"]["t"]
    print("[plev cancellation %s] t: spread %.3e .. %.3e" % (coord, spread.min(), spread.max()))
    assert 0.0 < spread.max() < 1e-5 and 200.0 < np.abs(ref["mean"]["t"]).min()
    compare("grid cancellation %s" % coord, got, ref, fields=pl.QUANTITIES)
    y = ref["members"]["t"]
    naive = np.sqrt(np.maximum((np.sum(y * y, axis=0) - 3 * np.mean(y, axis=0) ** 2) / 2, 0.0))
    assert pl.ulp_excess(naive.astype(np.float32), spread) > 1.0


# ------------------------------------------------------------------------------------------------ from spectra
CONFIGS = [("t30", 2), ("t30", 3), ("t30", 32), ("t63k16", 2)]
CONFIG_IDS = ["%s-E%d" % c for c in CONFIGS]


class Case:
    """one ensemble of E different members on the device and the oracle's FP64 grids of its members; made once per configuration"""

    def __init__(self, tag, E, oracle_factory):
        self.tag, self.E = tag, E
        self.sp, self.o = support.ensemble_plan(tag, E), oracle_factory(tag)
        self.sts = es.member_states(self.sp, E)
        self.ens, self.ins = eo.build(self.sp, self.o, self.sts)
        x = [eo.member_values(self.o, i) for i in self.ins]
        self.xe = {n: np.stack([m[n] for m in x]) for n in pl.QUANTITIES}
        self.ps = np.stack([self.o.spec_to_grid(i[5], 1) for i in self.ins])
        self.fsg = self.sp.table("fsg")
        self.scale = {n: float(np.max(np.abs(a))) for n, a in self.xe.items()}
        self.scale["ps"] = float(np.max(pl.P0 * np.exp(self.ps)))


def run(ens, plev, coord, **kw):
    import torch
    res = ens.output_pressure(plev, coord, **kw)
    torch.cuda.synchronize()
    return {g: (a.cpu().numpy() if g == "below" else {n: t.cpu().numpy() for n, t in a.items()}) for g, a in res.items()}


@pytest.fixture(scope="module")
def cases(oracle_factory):
    with support.plan_cache(lambda tag, E: Case(tag, E, oracle_factory), plan_of=lambda c: c.sp) as get:
        yield get


@pytest.mark.parametrize("tag,E", CONFIGS, ids=CONFIG_IDS)
def test_spectra_against_oracle(tag, E, cases):
    """1: members, mean and spread against the restatement on the oracle's FP64 grids, per point within 1e-12 (1 + 2A) scale + one
    float32 ulp of the reference value (a grid error of 1e-12 of scale in ps moves w by at most 2A times that, and |x[k+1] - x[k]| <=
    2 scale), on the reference script's eight levels, in both coordinates; `below` is the restatement's count"""
    c = cases(tag, E)
    A = pl.slope_factor(c.fsg)
    for coord in pl.COORDS:
        ref = pl.restate(c.fsg, c.xe, c.ps, pl.SCRIPT_LEVELS, coord)
        got = run(c.ens, pl.SCRIPT_LEVELS, coord, below=True)
        worst = 0.0
        for grp in GROUPS:
            for n in FIELDS:
                extra = 1e-12 * (1.0 if n == "ps" else 1.0 + 2.0 * A) * c.scale[n]
                ratio = pl.ulp_excess(got[grp][n], ref[grp][n], extra)
                worst = max(worst, ratio)
                assert ratio <= 1.0, (tag, E, coord, grp, n, ratio)
        print("[plev spectra %s E=%d %s] largest error / bound %.3g (A = %.2f)" % (tag, E, coord, worst, A))
        assert np.array_equal(got["below"], ref["below"].astype(np.float32)), (tag, E, coord)


def test_spectra_reference_route(cases):
    """2: the reference's route, linear mode, the script's eight levels: np.interp on Ensemble.output()'s float32 members in the
    script's float32 arithmetic.  Per point |device - script| <= 2 eps32 (max|f| + 6 (X/dX) |f[k+1] - f[k]|) for the bracket the
    restatement finds: twice the first-order bound of the float32 roundings of f, ps, sigma and the store"""
    import torch
    c = cases("t30", 2)
    snap = c.ens.output(stats=False)
    torch.cuda.synchronize()
    snap = eo.host(snap)["members"]
    got = run(c.ens, pl.SCRIPT_LEVELS, "p", stats=False)["members"]
    _, cls = pl.interpolate(c.fsg, c.xe, c.ps, pl.SCRIPT_LEVELS, "p")
    kb = cls["kb"]
    ratio_x = (c.fsg[1:] / np.diff(c.fsg))[kb]                                   # X_{k+1} / (X_{k+1} - X_k) of the bracket
    eps32 = float(np.finfo(np.float32).eps)
    sigma32 = c.fsg.astype(np.float32)
    worst = 0.0
    for n in pl.QUANTITIES:
        step = np.abs(np.diff(c.xe[n], axis=1))
        df = np.stack([np.take_along_axis(step[e], kb[e], axis=0) for e in range(c.E)])
        bound = 2.0 * eps32 * (c.scale[n] + 6.0 * ratio_x * df)
        for e in range(c.E):
            script = pl.script_route(snap[n][e], snap["ps"][e], sigma32, pl.SCRIPT_LEVELS)
            err = np.abs(got[n][e].astype(np.float64) - script.astype(np.float64))
            worst = max(worst, float(np.max(err / bound[e])))
            assert (err <= bound[e]).all(), (n, e, float(np.max(err / bound[e])))
    print("[plev reference route t30 E=2] largest error / bound %.3f" % worst)


def test_spectra_ps_fields_and_single_state(cases):
    """the three ps fields have the bits of Ensemble.output()'s, masked or not; the single-state call is bit-equal to member e of the
    ensemble call on that member's state (3)"""
    import torch
    c = cases("t30", 3)
    for use in (None, [1, 0, 1]):
        sig = c.ens.output(use=use)
        torch.cuda.synchronize()
        sig = eo.host(sig)
        for coord in pl.COORDS:
            got = run(c.ens, pl.SCRIPT_LEVELS, coord, use=use)
            for grp in GROUPS:
                assert support.same_bits(got[grp]["ps"], sig[grp]["ps"]), (use, coord, grp)
    lev = [85000.0, 50000.0, 101000.0]
    for coord in pl.COORDS:
        got = run(c.ens, lev, coord, stats=False)["members"]
        for e in range(c.E):
            dev = [torch.from_numpy(np.ascontiguousarray(a, np.complex128)).cuda() for a in c.ins[e]]
            outs = [torch.zeros((3, c.sp.il, c.sp.ix), dtype=torch.float32, device="cuda") for _ in range(5)]
            outs.append(torch.zeros((c.sp.il, c.sp.ix), dtype=torch.float32, device="cuda"))
            c.sp.output_pressure_dev(*dev, lev, coord, *outs)
            torch.cuda.synchronize()
            for n, a in zip(FIELDS, outs):
                assert support.same_bits(a.cpu().numpy(), got[n][e]), (coord, e, n)


def test_spectra_capture_and_determinism(cases):
    """4: captured after output_workspace with out= tensors and a device `use` it replays to the eager bits, in one node more than its
    inverse batch captured alone; two eager runs are bit-equal; only the mean, or only the members, wanted gives the bits of the full
    call; changing the host array of levels after the capture does not change a replay"""
    import torch
    c = cases("t30", 3)
    sp, ens, E, kx = c.sp, c.ens, c.E, c.sp.kx
    lev = np.array(pl.SCRIPT_LEVELS)
    nlev = len(lev)
    first, second = run(ens, lev, "p", below=True), run(ens, lev, "p", below=True)
    same = lambda a, b: all(support.same_bits(a[g][n], b[g][n]) for g in GROUPS for n in FIELDS) and support.same_bits(a["below"], b["below"])
    assert same(first, second)
    flat = lambda a: a.view((-1,) + tuple(a.shape[-2:]))
    new = lambda shapes: {n: torch.zeros(sh, dtype=torch.float32, device="cuda") for n, sh in shapes.items()}
    shapes = ens.output_pressure_shapes(nlev)
    ins = (ens.vor[0], ens.div[0], ens.t[0], ens.tr[0], ens.phi, ens.ps[0])
    only_mean, only_members = new(shapes["mean"]), new(shapes["members"])
    sp.ens_output_pressure_dev(E, *ins, lev, "p", mean=only_mean)
    sp.ens_output_pressure_dev(E, *ins, lev, "p", members=only_members)
    torch.cuda.synchronize()
    for n in FIELDS:
        assert support.same_bits(only_mean[n].cpu().numpy(), first["mean"][n]), n
        assert support.same_bits(only_members[n].cpu().numpy(), first["members"][n]), n
    # the capture
    out = {g: new(shapes[g]) for g in GROUPS}
    out["below"] = torch.zeros(shapes["below"], dtype=torch.float32, device="cuda")
    use = torch.ones(E, dtype=torch.int32, device="cuda")
    ug, vg = (torch.zeros((E * kx, sp.il, sp.ix), dtype=torch.float64, device="cuda") for _ in range(2))
    plain = torch.zeros((3 * E * kx + E, sp.il, sp.ix), dtype=torch.float64, device="cuda")
    ens.output_workspace()
    sp.use_own_stream()
    torch.cuda.synchronize()
    try:
        with sp.graph_capture() as g:
            res = ens.output_pressure(lev, "p", use=use, below=True, out=out)
        with sp.graph_capture() as g_inv:
            sp.inverse_batch_segs_dev(flat(ens.vor[0]), flat(ens.div[0]), ug, vg,
                                      [flat(ens.t[0]), flat(ens.tr[0]), flat(ens.phi), ens.ps[0]], plain, kcos_pairs=2, kcos=1)
        assert all(res[grp][n] is out[grp][n] for grp in GROUPS for n in FIELDS) and res["below"] is out["below"]
        assert g.num_nodes() == g_inv.num_nodes() + 1, (g.num_nodes(), g_inv.num_nodes())
        lev[:] = lev[::-1] * 0.5                                    # the captured call keeps the values it was enqueued with
        for _ in range(2):
            g.launch()
        sp.synchronize()
        replay = {grp: {n: out[grp][n].cpu().numpy() for n in FIELDS} for grp in GROUPS}
        replay["below"] = out["below"].cpu().numpy()
        assert same(replay, first)
        g.close(); g_inv.close()
    finally:
        sp.use_torch_stream()
    third = run(ens, pl.SCRIPT_LEVELS, "p", below=True)
    assert same(third, first)
