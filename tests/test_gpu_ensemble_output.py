"""GPU: the ensemble output (include/spdy.h "ensemble output", Ensemble.output) -- every member's float32 snapshot,
the ensemble mean and the spread from one call.  The members have DIFFERENT states.  A member's fields are held to the
single-state call on that member's state (bit for bit at T30, where a field's bits do not depend on its batch) and to the oracle's
output; mean and spread to the longdouble statistics of the oracle's FP64 grids (tests/ensembleoutput.py)."""
import numpy as np
import pytest

import ensembleoutput as eo
import ensemblestep as es
import support

pytestmark = pytest.mark.gpu

CONFIGS = [("t30", 3), ("t30k5", 3), ("t30", 17), ("t63k16", 2)]     # kx = 5: tiles of two fields straddle members; E = 17: the
CONFIG_IDS = ["%s-E%d" % c for c in CONFIGS]                        # transform leaves the model-sized form; T63 L16: launch forms (s8)
GROUPS = ("members", "mean", "spread")


class Case:
    """one ensemble of E different members on the device, its full output, and the reference side; made once per configuration"""

    def __init__(self, tag, E, oracle_factory):
        self.tag, self.E = tag, E
        self.sp, self.o = support.ensemble_plan(tag, E), oracle_factory(tag)
        self.sts = es.member_states(self.sp, E)
        self.ens, self.ins = eo.build(self.sp, self.o, self.sts)
        self.got = run(self.ens)
        self.x = [eo.member_values(self.o, i) for i in self.ins]
        self.mean, self.spread, self.scale = eo.statistics(self.x)


def run(ens, **kw):
    import torch
    res = ens.output(**kw)
    torch.cuda.synchronize()
    return eo.host(res)


@pytest.fixture(scope="module")
def cases(oracle_factory):
    with support.plan_cache(lambda tag, E: Case(tag, E, oracle_factory), plan_of=lambda c: c.sp) as get:
        yield get


@pytest.mark.parametrize("tag,E", CONFIGS, ids=CONFIG_IDS)
def test_members(tag, E, cases):
    """(a) every member's six fields against spdy_output_batch_dev on that member's state -- bit-equal at T30, within one float32
    ulp at T63 L16 where the launch form may differ -- and within one float32 ulp of the oracle's output on that member"""
    c = cases(tag, E)
    for e in range(E):
        single = eo.single_output(c.sp, c.ins[e])
        ref = dict(zip(eo.FIELDS, c.o.output(*c.ins[e])))
        for n in eo.FIELDS:
            mine = c.got["members"][n][e]
            d_single, d_ref = eo.ulps(mine, single[n]), eo.ulps(mine, ref[n])
            print("[ens output %s E=%d] member %d %s: %d ulp from the single call, %d from the oracle" % (tag, E, e, n, d_single, d_ref))
            if tag.startswith("t30"):
                assert support.same_bits(mine, single[n]), (e, n)
            assert d_single <= 1 and d_ref <= 1, (e, n, d_single, d_ref)


@pytest.mark.parametrize("tag,E", CONFIGS, ids=CONFIG_IDS)
def test_statistics(tag, E, cases):
    """(b) mean and spread of every quantity: |device - float32(ref)| <= 1e-12 max|x| + one float32 ulp of the reference value"""
    c = cases(tag, E)
    for grp, ref in (("mean", c.mean), ("spread", c.spread)):
        for n in eo.FIELDS:
            assert c.got[grp][n].dtype == np.float32 and c.got[grp][n].shape == ref[n].shape
            excess = eo.within(c.got[grp][n], ref[n], c.scale[n])
            print("[ens output %s E=%d] %s %s: excess over the bound %.3e (scale %.3e)" % (tag, E, grp, n, excess, c.scale[n]))
            assert excess <= 0.0, (grp, n, excess)


def test_one_member(cases):
    """(b) E = 1: the mean is the member's output, bit for bit, and the spread exactly +0"""
    c = cases("t30", 1)
    for n in eo.FIELDS:
        assert support.same_bits(c.got["mean"][n], c.got["members"][n][0]), n
        assert not c.got["spread"][n].view(np.int32).any(), n
        assert support.same_bits(c.got["members"][n][0], eo.single_output(c.sp, c.ins[0])[n]), n


def poisoned(c):
    """c's ensemble with member 1 poisoned as tests/test_gpu_isolation.py does: every prognostic (and its phi) NaN, ps +inf"""
    nan, inf = float("nan"), float("inf")
    ens, _ = eo.build(c.sp, c.o, c.sts)
    for n in ("vor", "div", "t", "tr"):
        getattr(ens, n)[:, 1] = complex(nan, nan)
    ens.phi[1] = complex(nan, nan)
    ens.ps[:, 1] = complex(inf, 0.0)
    return ens


def test_mask_and_isolation(cases):
    """(c) T30, kx = 5, E = 3, member 1 NaN with ps +inf.  Members 0 and 2 keep the clean run's bits; with member 1 masked out the
    statistics are those of the E = 2 ensemble of members 0 and 2, bit for bit; unmasked they are NaN.  On clean members one member
    in use gives its own output and spread +0, none in use NaN."""
    c = cases("t30k5", 3)
    bad = poisoned(c)
    masked, unmasked = run(bad, use=[1, 0, 1]), run(bad)
    two, _ = eo.build(c.sp, c.o, [c.sts[0], c.sts[2]])
    pair = run(two)
    for n in eo.FIELDS:
        for got in (masked, unmasked):
            for e in (0, 2):
                assert support.same_bits(got["members"][n][e], c.got["members"][n][e]), (n, e)
        for grp in ("mean", "spread"):
            assert support.same_bits(masked[grp][n], pair[grp][n]), (grp, n)
            assert np.isfinite(masked[grp][n]).all(), (grp, n)
            if n != "ps":
                assert np.isnan(unmasked[grp][n]).all(), (grp, n)
    # the mask is the same whether it comes as a sequence or as a device tensor
    import torch
    again = run(bad, use=torch.tensor([7, 0, -1], dtype=torch.int32, device="cuda"))
    assert all(support.same_bits(again[g][n], masked[g][n]) for g in ("mean", "spread") for n in eo.FIELDS)
    one, none = run(c.ens, use=[0, 1, 0]), run(c.ens, use=[0, 0, 0])
    for n in eo.FIELDS:
        assert support.same_bits(one["mean"][n], c.got["members"][n][1]), n
        assert not one["spread"][n].view(np.int32).any(), n
        assert np.isnan(none["mean"][n]).all() and np.isnan(none["spread"][n]).all(), n
        assert support.same_bits(none["members"][n], c.got["members"][n]), n          # the members are written whatever the mask says


def test_cancellation(cases, oracle_factory):
    """(d) T30, kx = 8, E = 3: member e's t is grid_to_spec(288 + 1e-6 r_e) per level, r_e seeded standard-normal grids -- a spread
    near 1e-6 on a mean of 288.  The spread of t must meet (b)'s bound, 1e-12 * 288 = 2.9e-10: two passes leave 1e-17, Welford
    4e-14, the one-pass sum of squares 7e-6 (and a negative variance at more than half the points)."""
    c = cases("t30", 3)
    sp, o = c.sp, c.o
    sts = [dict(st) for st in c.sts]
    for e, st in enumerate(sts):
        r = np.random.default_rng(4200 + e).standard_normal((sp.kx, sp.il, sp.ix))
        t = np.array(st["t"], copy=True)
        t[0] = np.stack([o.grid_to_spec(288.0 + 1e-6 * r[k]) for k in range(sp.kx)])
        st["t"] = t
    ens, ins = eo.build(sp, o, sts, phis=[i[4] for i in c.ins])     # the other prognostics, and phi, as in (a)
    got = run(ens, members=False)
    mean, spread, scale = eo.statistics([eo.member_values(o, i) for i in ins])
    print("[ens output cancellation] t: max|x| %.6f, spread %.3e .. %.3e" % (scale["t"], spread["t"].min(), spread["t"].max()))
    assert 280.0 < scale["t"] < 300.0 and 1e-7 < spread["t"].max() < 1e-5     # (the round trip of a constant is 287.1 .. 293.3)
    for grp, ref in (("mean", mean), ("spread", spread)):
        for n in eo.FIELDS:
            excess = eo.within(got[grp][n], ref[n], scale[n])
            print("[ens output cancellation] %s %s: excess over the bound %.3e" % (grp, n, excess))
            assert excess <= 0.0, (grp, n, excess)
    # the bound does tell the algorithms apart here: the sum-of-squares form, evaluated in FP64 on the same values, misses it
    x = np.stack([eo.member_values(o, i)["t"] for i in ins])
    naive = np.sqrt(np.maximum((np.sum(x * x, axis=0) - 3 * np.mean(x, axis=0) ** 2) / 2, 0.0))
    assert eo.within(naive.astype(np.float32), spread["t"], scale["t"]) > 0.0


def test_capture_and_determinism(cases):
    """(e) captured after output_workspace with out= tensors it replays to the eager bits, in one node more than its inverse batch
    captured alone; two eager runs are bit-equal; only the mean, or only the members, wanted gives the bits of the full call"""
    import torch
    import speedy_f90_amd as s
    c = cases("t30", 3)
    sp, ens, E, kx = c.sp, c.ens, c.E, c.sp.kx
    second = run(ens)
    for g in GROUPS:
        for n in eo.FIELDS:
            assert support.same_bits(second[g][n], c.got[g][n]), (g, n)
    flat = lambda a: a.view((-1,) + tuple(a.shape[-2:]))
    new = lambda shapes: {n: torch.zeros(sh, dtype=torch.float32, device="cuda") for n, sh in shapes.items()}
    shapes = ens.output_shapes()
    # single groups through the C call's NULL structs
    ins = (ens.vor[0], ens.div[0], ens.t[0], ens.tr[0], ens.phi, ens.ps[0])
    only_mean, only_members = new(shapes["mean"]), new(shapes["members"])
    sp.ens_output_batch_dev(E, *ins, mean=only_mean)
    sp.ens_output_batch_dev(E, *ins, members=only_members)
    torch.cuda.synchronize()
    for n in eo.FIELDS:
        assert support.same_bits(only_mean[n].cpu().numpy(), c.got["mean"][n]), n
        assert support.same_bits(only_members[n].cpu().numpy(), c.got["members"][n]), n
    # the capture
    out = {g: new(shapes[g]) for g in GROUPS}
    use = torch.ones(E, dtype=torch.int32, device="cuda")
    ug, vg = (torch.zeros((E * kx, sp.il, sp.ix), dtype=torch.float64, device="cuda") for _ in range(2))
    plain = torch.zeros((3 * E * kx + E, sp.il, sp.ix), dtype=torch.float64, device="cuda")
    ens.output_workspace()
    sp.use_own_stream()
    torch.cuda.synchronize()
    try:
        with sp.graph_capture() as g:
            res = ens.output(use=use, out=out)
        with sp.graph_capture() as g_inv:
            sp.inverse_batch_segs_dev(flat(ens.vor[0]), flat(ens.div[0]), ug, vg,
                                      [flat(ens.t[0]), flat(ens.tr[0]), flat(ens.phi), ens.ps[0]], plain, kcos_pairs=2, kcos=1)
        assert all(res[grp][n] is out[grp][n] for grp in GROUPS for n in eo.FIELDS)
        assert g.num_nodes() == g_inv.num_nodes() + 1, (g.num_nodes(), g_inv.num_nodes())
        for _ in range(2):
            g.launch()
        sp.synchronize()
        for grp in GROUPS:
            for n in eo.FIELDS:
                assert support.same_bits(out[grp][n].cpu().numpy(), c.got[grp][n]), (grp, n)
        # the workspace cannot grow inside a capture: SPDY_ERR_STATE, and the plan goes on working
        with pytest.raises(s.SpdyError) as err:
            with sp.graph_capture():
                sp.ens_output_workspace(E + 1)
        assert err.value.code == -5
        g.close(); g_inv.close()
    finally:
        sp.use_torch_stream()
    third = run(ens)
    assert all(support.same_bits(third[grp][n], c.got[grp][n]) for grp in GROUPS for n in eo.FIELDS)
