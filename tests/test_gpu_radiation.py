"""GPU: radiation on the device (csrc/spdy_radiation.hip; physics.f90:146-166, :180-186) -- against the flang-built reference's
fixture, the step without shortwave on a held state, batch composition, the chain moist -> down -> surface -> up plain and
captured, a new date between two replays, and the argument checks."""
import os

import numpy as np
import pytest

import moist
import radiation
import support
import synth
from conftest import GOLDEN, TOL

pytestmark = pytest.mark.gpu

ZON = ("fsol", "ozone", "ozupp", "zenit", "stratz")


def _g(c, n, il, ix):
    return radiation.grids(c[n], 1, il, ix)[0]


def _assert_close(got, want, key):
    if key.endswith("icltop"):
        assert np.array_equal(got, want), key
        return 0.0
    e = synth.relerr(got, want)
    assert e <= TOL, (key, e)
    return e


@pytest.mark.parametrize("tag", support.PHYSICS_TAGS)
def test_radiation_columns_vs_reference(tag):
    """radiation_columns with every optional output against the reference at both dates (integers identical, floats within TOL),
    then the step without shortwave on the held state against the reference and the restatement."""
    z = np.load(os.path.join(GOLDEN, "ref_radiation.npz"))
    ix, il, kx = support.grid(tag)
    ncol = il * ix
    tab = moist.tables(moist.HSG[kx])
    zon0 = radiation.zonal_columns({n: z["%s_d0_%s" % (tag, n)] for n in ZON}, 1, il, ix)
    c = radiation.columns(tab, ncol, int(z[tag + "_seed"]), zon0)
    sub = z[tag + "_sub"]
    G = lambda n: _g(c, n, il, ix)
    sp = support.plan(tag)
    worst = 0.0
    for di, ty in enumerate(radiation.DATES):
        sp.radiation_set_date(ty)
        r1 = sp.radiation_columns(G("tg"), G("qg"), G("phig"), G("pslg"), G("rh"), G("precnv"), G("precls"), G("iptop"),
                                  G("fmask"), G("albsfc"), G("ts"), G("fsfcu"), G("ttend_m"), compute_sw=True)
        for n in radiation.SW_OUT + ("icltop",):
            worst = max(worst, _assert_close(radiation.cols(r1[n][None])[..., sub], z["%s_d%d_s1_%s" % (tag, di, n)], n))
        r2 = sp.radiation_columns(G("tg2"), G("qg"), G("phig"), G("pslg"), None, None, None, None, None, None, G("ts2"),
                                  G("fsfcu2"), G("ttend2"), compute_sw=False, state=r1["state"])
        for n in radiation.NOSW_OUT:
            worst = max(worst, _assert_close(radiation.cols(r2[n][None])[..., sub], z["%s_d%d_s2_%s" % (tag, di, n)], n))
        # every column of the step without shortwave against the restatement with the held state
        zon = radiation.zonal_columns({n: z["%s_d%d_%s" % (tag, di, n)] for n in ZON}, 1, il, ix)
        _, q2 = radiation.two_steps(tab, c, zon)
        for n in radiation.NOSW_OUT:
            worst = max(worst, _assert_close(radiation.cols(r2[n][None]), q2[n], n))
    sp.close()
    print("\n[radiation columns %s vs reference] worst %.1e" % (tag, worst))


def _inputs(tab, nb, il, ix, seed, sp):
    """nb states of columns as device grids: (dict of tensors, restated columns, zonal per column)"""
    zl = {n: sp.table(n) for n in ZON}
    zon = radiation.zonal_columns(zl, nb, il, ix)
    c = radiation.columns(tab, nb * il * ix, seed, zon)
    d = {n: support.dev(radiation.grids(c[n], nb, il, ix)) for n in c if n != "iptop"}
    d["iptop"] = support.dev(radiation.grids(c["iptop"], nb, il, ix).astype(np.int32))
    return d, c, zon


def _run(sp, d, nb, st, T, out, sw=True):
    sp.radiation_down_dev(sw, d["tg"], d["qg"], d["phig"], d["pslg"], d["rh"], d["precnv"], d["precls"], d["iptop"], d["fmask"],
                          d["albsfc"], st, out)
    sp.radiation_up_dev(d["tg"], d["pslg"], d["ts"], d["fsfcu"], st, T, out)


def test_batch_composition_and_null_outputs():
    """A state's output bits do not depend on nb or on its position in the batch; NULL outputs leave ttend and the state
    bit-equal."""
    import torch
    sp = support.plan("t30", 64)
    sp.radiation_set_date(radiation.DATES[0])
    ix, il, kx = support.grid("t30")
    tab = moist.tables(moist.HSG[kx])
    S = sp.radiation_state_size()
    for nb in (1, 5, 64):
        d, _, _ = _inputs(tab, nb, il, ix, 9300 + nb, sp)
        st = torch.zeros(nb * S, dtype=torch.float64, device="cuda")
        T, out = d["ttend_m"].clone(), sp.column_outputs(nb, "rad")
        _run(sp, d, nb, st, T, out)
        st0 = torch.zeros_like(st)
        T0 = d["ttend_m"].clone()
        _run(sp, d, nb, st0, T0, None)
        torch.cuda.synchronize()
        assert torch.equal(T, T0) and torch.equal(st, st0)
        for b in sorted({0, nb // 2, nb - 1}):
            one = {n: v[b:b + 1].contiguous() for n, v in d.items()}
            s1 = torch.zeros(S, dtype=torch.float64, device="cuda")
            T1, o1 = one["ttend_m"].clone(), sp.column_outputs(1, "rad")
            _run(sp, one, 1, s1, T1, o1)
            torch.cuda.synchronize()
            assert torch.equal(T1[0], T[b]), (nb, b)
            assert torch.equal(s1, st[b * S:(b + 1) * S]), (nb, b)
            for n in o1:
                assert torch.equal(o1[n][0], out[n][b]), (nb, b, n)
    sp.close()


@pytest.mark.parametrize("tag", ["t30", "t63k16"])
def test_chain_capture_and_date(tag):
    """moist_columns_dev -> radiation_down_dev -> the caller's ts / fsfcu -> radiation_up_dev (then a step without shortwave)
    matches the restatement; the same sequence captured and replayed is bit-equal to the plain launches; spdy_radiation_set_date
    between two replays changes the replayed result to the new date's."""
    import torch
    nb = 2
    sp = support.plan(tag, 64)
    ix, il, kx = support.grid(tag)
    tab = moist.tables(moist.HSG[kx])
    sp.radiation_set_date(radiation.DATES[0])
    d, c, zon = _inputs(tab, nb, il, ix, 9400, sp)
    S = sp.radiation_state_size()

    def seq(D):
        sp.moist_columns_dev(D["tg"], D["qg"], D["phig"], D["pslg"], D["T"], D["Q"], D["mo"])
        sp.radiation_down_dev(True, D["tg"], D["qg"], D["phig"], D["pslg"], D["mo"]["rh"], D["mo"]["precnv"], D["mo"]["precls"],
                              D["mo"]["iptop"], D["fmask"], D["albsfc"], D["st"], D["out"])
        sp.radiation_up_dev(D["tg"], D["pslg"], D["ts"], D["fsfcu"], D["st"], D["T"], D["out"])
        sp.radiation_down_dev(False, D["tg2"], D["qg"], D["phig"], D["pslg"], None, None, None, None, None, None, D["st"], D["out2"])
        sp.radiation_up_dev(D["tg2"], D["pslg"], D["ts2"], D["fsfcu2"], D["st"], D["T2"], D["out2"])

    def fresh():
        D = {n: d[n] for n in ("tg", "qg", "phig", "pslg", "fmask", "albsfc", "ts", "fsfcu", "tg2", "ts2", "fsfcu2")}
        D["T"], D["Q"], D["T2"] = d["ttend"].clone(), d["qtend"].clone(), d["ttend2"].clone()
        D["mo"] = sp.column_outputs(nb, "moist", names=("precnv", "precls", "iptop", "rh"))
        D["st"] = torch.full((nb * S,), float("nan"), dtype=torch.float64, device="cuda")
        D["out"], D["out2"] = sp.column_outputs(nb, "rad"), sp.column_outputs(nb, "rad")
        return D

    P = fresh()
    seq(P)
    torch.cuda.synchronize()
    r1, r2 = radiation.two_steps(tab, c, zon)
    worst = 0.0
    for n in radiation.SW_OUT + ("icltop",):
        got = P["T"] if n == "ttend" else P["out"][n]
        worst = max(worst, _assert_close(radiation.cols(got.cpu().numpy()), r1[n], n))
    for n in radiation.NOSW_OUT:
        got = P["T2"] if n == "ttend" else P["out2"][n]
        worst = max(worst, _assert_close(radiation.cols(got.cpu().numpy()), r2[n], n))
    print("\n[radiation chain %s vs restatement] worst %.1e" % (tag, worst))

    # captured and replayed: bit-equal to the plain launches
    D = fresh()
    torch.cuda.synchronize()
    with sp.graph_capture() as g:
        seq(D)
    g.launch()
    sp.synchronize()
    for n in ("T", "T2", "st"):
        assert torch.equal(D[n], P[n]), n
    for n in P["out"]:
        assert torch.equal(D["out"][n], P["out"][n]) and torch.equal(D["out2"][n], P["out2"][n]), n
    # a new date between two replays: the replay follows it
    sp.radiation_set_date(radiation.DATES[1])
    for n, v in fresh().items():
        if isinstance(v, dict):
            for m, w in v.items():
                D[n][m].copy_(w)
        elif n in ("T", "Q", "T2", "st"):
            D[n].copy_(v)
    torch.cuda.synchronize()
    g.launch()
    sp.synchronize()
    zon1 = radiation.zonal_columns({n: sp.table(n) for n in ZON}, nb, il, ix)
    q1, _ = radiation.two_steps(tab, c, zon1)
    for n in ("tsr", "ssrd", "tt_rsw"):
        got = radiation.cols(D["out"][n].cpu().numpy())
        _assert_close(got, q1[n], n)
        assert not np.array_equal(got, radiation.cols(P["out"][n].cpu().numpy())), n
    _assert_close(radiation.cols(D["T"].cpu().numpy()), q1["ttend"], "ttend")
    g.close()
    sp.close()


def test_argument_checks_and_index_clamp():
    """The error codes of the C ABI on a device plan, and temperatures outside the table (the fband index clamp) giving finite
    values equal to the clamped restatement."""
    import torch
    import speedy_f90_amd as s
    sp = support.plan("t30", 8)
    ix, il, kx = support.grid("t30")
    tab = moist.tables(moist.HSG[kx])
    S = sp.radiation_state_size()
    st = torch.zeros(S, dtype=torch.float64, device="cuda")
    g3 = torch.zeros((1, kx, il, ix), dtype=torch.float64, device="cuda")
    g2 = torch.zeros((1, il, ix), dtype=torch.float64, device="cuda")
    i2 = torch.zeros((1, il, ix), dtype=torch.int32, device="cuda")
    with pytest.raises(s.SpdyError) as e:                     # no date yet
        sp.radiation_down_dev(True, g3, g3, g3, g2, g3, g2, g2, i2, g2, g2, st)
    assert e.value.code == -5
    with pytest.raises(s.SpdyError) as e:
        sp.radiation_up_dev(g3, g2, g2, g2, st, g3)
    assert e.value.code == -5
    sp.radiation_set_date(0.3)
    with pytest.raises(s.SpdyError) as e:                     # NULL rh with compute_sw
        sp.radiation_down_dev(True, g3, g3, g3, g2, None, g2, g2, i2, g2, g2, st)
    assert e.value.code == -1
    lib = sp.lib
    assert lib.spdy_radiation_down_dev(sp.h, 9, 1, *[None] * 8, None, None, None) == -1    # nb > max_batch
    sp.close()
    sp = s.Spectral("t30", kx=17, max_batch=8, device=0)
    assert lib.spdy_radiation_state_size(sp.h) == -1
    sp.close()

    # out-of-range temperatures: the index is clamped to [100, 400] (rows 200 / 320 of the table)
    sp = support.plan("t30", 8)
    sp.radiation_set_date(radiation.DATES[1])
    zon = radiation.zonal_columns({n: sp.table(n) for n in ZON}, 1, il, ix)
    c = radiation.columns(tab, il * ix, 9500, zon)
    u = synth.splitmix64(9501, kx * il * ix).reshape(kx, il * ix)
    for n, lo, hi in (("tg", 20.0, 700.0), ("tg2", 20.0, 700.0)):
        c[n] = lo + (hi - lo) * u
    c["ts"] = 20.0 + 680.0 * u[0]
    c["ts2"] = 20.0 + 680.0 * u[1]
    r1, r2 = radiation.two_steps(tab, c, zon)
    G = lambda n: _g(c, n, il, ix)
    g1 = sp.radiation_columns(G("tg"), G("qg"), G("phig"), G("pslg"), G("rh"), G("precnv"), G("precls"), G("iptop"), G("fmask"),
                              G("albsfc"), G("ts"), G("fsfcu"), G("ttend_m"))
    g2_ = sp.radiation_columns(G("tg2"), G("qg"), G("phig"), G("pslg"), None, None, None, None, None, None, G("ts2"),
                               G("fsfcu2"), G("ttend2"), compute_sw=False, state=g1["state"])
    for n in ("slrd", "slr", "olr", "tt_rlw", "ttend"):
        for got, want in ((g1[n], r1[n]), (g2_[n], r2[n])):
            assert np.all(np.isfinite(got)), n
            _assert_close(radiation.cols(got[None]), want, n)
    sp.close()
