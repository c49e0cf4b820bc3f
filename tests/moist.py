"""Moist physics of the column: the precipitation block of get_physical_tendencies (physics.f90:110-138) restated in NumPy, its
tables (physics.f90:12-39, convection.f90:55-71, large_scale_condensation.f90:47-66), seeded physically shaped columns to run it
on, and a physics hook for dynstep.oracle_dynamics_step.  Pinned to the flang-built reference by tests/golden/ref_moist.npz
(tests/golden/make_golden_moist.py); the device kernel (csrc/spdy_physics.hip) is checked against both.

Arrays are NumPy C-order views of the reference's column-major ones: a level stack (ix,il,kx) is [kx, il, ix]; the restatement
works on [kx, ncol] (any number of columns), vectorised over columns and looping over k as the reference does.  Default-real
literals of the reference are float32 values widened to double: f32(x) below."""
import contextlib

import numpy as np

import synth


def f32(x):
    return float(np.float32(x))


# physical_constants.f90:16-26, humidity.f90:61-66, convection.f90:15-22, large_scale_condensation.f90:24-27
GRAV, P0, CP, ALHC = f32(9.81), f32(1.e+5), f32(1004.0), f32(2501.0)
E0, C1, C2, T0, T1, T2 = 6.108e-3, f32(17.269), f32(21.875), f32(273.16), f32(35.86), f32(7.66)
PSMIN, TRCNV, RHBL, RHIL, ENTMAX, SMF = f32(0.8), f32(6.0), f32(0.9), f32(0.7), f32(0.5), f32(0.8)
TRLSC, RHLSC, DRHLSC, RHBLSC = f32(4.0), f32(0.9), f32(0.1), f32(0.95)
LOG099 = float(np.array([0xBC24AA20], np.uint32).view(np.float32)[0])   # physics.f90:37: log(0.99) of a default real = float32 logf
# (pinned: a libm float32 log may differ in its last bits; the reference's is -1.00503265857696533e-2)

# geometry.f90:42-48 (float32 literals) and the 16-level set of tests/synth.py
HSG = {5: np.array([0.000, 0.150, 0.350, 0.650, 0.900, 1.000], np.float32).astype(np.float64),
       7: np.array([0.020, 0.140, 0.260, 0.420, 0.600, 0.770, 0.900, 1.000], np.float32).astype(np.float64),
       8: np.array([0.000, 0.050, 0.140, 0.260, 0.420, 0.600, 0.770, 0.900, 1.000], np.float32).astype(np.float64),
       16: synth.SIGMA_L16}


def tables(hsg):
    """Everything the block reads that depends on the levels only: geometry.f90:51-53 (dhs, fsg), physics.f90:12-39 (sigl, sigh,
    grdsig, grdscp, wvi [2, kx] = wvi(kx,2) transposed), convection.f90:55-71 (entr(2:kx-1), fm0)."""
    hsg = np.asarray(hsg, np.float64)
    kx = hsg.size - 1
    dhs = hsg[1:] - hsg[:-1]
    fsg = 0.5 * (hsg[1:] + hsg[:-1])
    sigl = np.log(fsg)
    sigh = hsg.copy()
    grdsig = GRAV / (dhs * P0)
    grdscp = grdsig / CP
    wvi = np.zeros((2, kx))
    wvi[0, :-1] = 1.0 / (sigl[1:] - sigl[:-1])
    wvi[1, :-1] = (np.log(sigh[1:kx]) - sigl[:-1]) * wvi[0, :-1]
    wvi[1, kx - 1] = (LOG099 - sigl[kx - 1]) * wvi[0, kx - 2]
    fm0 = P0 * dhs[kx - 1] / (GRAV * TRCNV * 3600.0)
    entr = np.maximum(0.0, fsg[1:kx - 1] - 0.5) ** 2
    sentr = 0.0
    for e in entr:
        sentr = sentr + e
    entr = entr * (ENTMAX / sentr)
    return {"kx": kx, "hsg": hsg, "dhs": dhs, "fsg": fsg, "sigl": sigl, "sigh": sigh, "grdsig": grdsig, "grdscp": grdscp,
            "wvi": wvi, "entr": entr, "fm0": fm0}


def get_qsat(ta, ps, sig):
    """humidity.f90:46-79 (sig > 0)."""
    x = np.where(ta >= T0, C1 * (ta - T0) / (ta - T1), C2 * (ta - T0) / (ta - T2))
    q = E0 * np.exp(x)
    return 622.0 * q / (sig * ps - f32(0.378) * q)


# Ties.  A NEAR tie (0 < margin < MIN_MARGIN) of a decision with a computed side is one the device and the reference may decide
# differently, and the column is always drawn again.  A decision whose two sides are bit-identical on the device and in the
# reference (inputs, literals, results of clamps: class (i) of tests/thresholds.py, marked exact=True below) is fully determined
# by the reference's operator AT the tie and one ulp next to it.  By default such a decision is held to the margin rule like any
# other, so an exact tie (margin 0) is drawn again with the near ones: the drawn columns of the committed fixtures.  Inside
# `with exact_ties():` a class-(i) decision reports no margin at all (inf), so that columns constructed ON a threshold and on its
# one-ulp neighbours survive the redraw rule, which goes on removing the near ties of every other decision.
EXACT_TIES = False


@contextlib.contextmanager
def exact_ties():
    global EXACT_TIES
    old, EXACT_TIES = EXACT_TIES, True
    try:
        yield
    finally:
        EXACT_TIES = old


def _margin(a, b, exact=False):
    """relative distance of a decision a > b (or a >= b, a < b) from its tie; exact=True marks a class-(i) decision, which inside
    exact_ties() is clear (inf) wherever it stands"""
    if exact and EXACT_TIES:
        return np.full(np.broadcast(a, b).shape, np.inf)
    s = np.maximum(np.abs(a), np.abs(b))
    return np.where(s > 0, np.abs(a - b) / np.where(s > 0, s, 1.0), np.inf)


def column_block(tab, tg, qg, phig, pslg, ttend, qtend):
    """physics.f90:110-138 on [kx, ncol] columns (pslg [ncol]).  Returns the updated ttend, qtend and every optional output
    (precnv, precls, cbmf, iptop, icnv [ncol]; qsat, rh, se [kx, ncol]), plus `margin` [ncol]: the smallest relative distance of
    any decision of the column from its threshold (psa > psmin, mss0 > mss2, mse1 > mss2, qa > qthr, delq > 0, dqa < 0,
    ta >= t0), and `branch` counts."""
    kx = tab["kx"]
    fsg, dhs, wvi, entr = tab["fsg"], tab["dhs"], tab["wvi"][1], tab["entr"]
    E = lambda k: entr[k - 2]                                    # entr(2:kx-1)
    W = lambda k: wvi[k - 1]                                     # wvi(k,2)
    tg, phig = np.asarray(tg, np.float64), np.asarray(phig, np.float64)
    n = tg.shape[1]
    margin = np.full(n, np.inf)

    # thermodynamic fields (physics.f90:110-119)
    psg = np.exp(pslg)
    rps = 1.0 / psg
    clamped = np.any(qg < 0.0, axis=0)
    qa = np.maximum(qg, 0.0)
    se = CP * tg + phig
    qsat = np.stack([get_qsat(tg[k], psg, fsg[k]) for k in range(kx)])
    rh = qa / qsat
    warm = tg >= T0
    margin = np.minimum(margin, np.min(_margin(tg, np.full_like(tg, T0), exact=True), axis=0))

    # diagnose_convection (convection.f90:158-235)
    nl1, nlp = kx - 1, kx + 1
    mss = se + ALHC * qsat                                      # used for k = 2..kx
    itop = np.full(n, nlp, np.int64)
    qdif = np.zeros(n)
    live = psg > PSMIN
    margin = np.minimum(margin, _margin(psg, np.full(n, PSMIN)))
    mse0 = se[kx - 1] + ALHC * qa[kx - 1]
    mse1 = np.minimum(mse0, se[nl1 - 1] + ALHC * qa[nl1 - 1])
    mss0 = np.maximum(mse0, mss[kx - 1])
    ktop1 = np.full(n, kx, np.int64)
    ktop2 = np.full(n, kx, np.int64)
    msthr = np.zeros(n)
    for k in range(kx - 3, 2, -1):
        mss2 = mss[k - 1] + W(k) * (mss[k] - mss[k - 1])
        c1 = mss0 > mss2
        c2 = mse1 > mss2
        margin = np.where(live, np.minimum(margin, np.minimum(_margin(mss0, mss2), _margin(mse1, mss2))), margin)
        ktop1 = np.where(c1, k, ktop1)
        ktop2 = np.where(c2, k, ktop2)
        msthr = np.where(c2, mss2, msthr)
    qthr0 = RHBL * qsat[kx - 1]
    qthr1 = RHBL * qsat[nl1 - 1]
    lqthr = (qa[kx - 1] > qthr0) & (qa[nl1 - 1] > qthr1)
    cond = live & (ktop1 < kx)
    margin = np.where(cond, np.minimum(margin, np.minimum(_margin(qa[kx - 1], qthr0), _margin(qa[nl1 - 1], qthr1))), margin)
    via2 = cond & (ktop2 < kx)
    via_q = cond & (ktop2 >= kx) & lqthr
    itop = np.where(via2 | via_q, ktop1, itop)
    qdif = np.where(via2, np.maximum(qa[kx - 1] - qthr0, (mse0 - msthr) * (1.0 / ALHC)), qdif)
    qdif = np.where(via_q, qa[kx - 1] - qthr0, qdif)

    # mass fluxes (convection.f90:74-152), all columns at once, masked by conv
    conv = itop != nlp
    rdps = 2.0 / (1.0 - PSMIN)
    dfse = np.zeros((kx, n))
    dfqa = np.zeros((kx, n))
    cbmf = np.zeros(n)
    precnv = np.zeros(n)
    sec_flux = np.zeros(n, bool)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        k = kx
        k1 = k - 1
        qmax = np.maximum(f32(1.01) * qa[k - 1], qsat[k - 1])
        sb = se[k1 - 1] + W(k1) * (se[k - 1] - se[k1 - 1])
        qb = qa[k1 - 1] + W(k1) * (qa[k - 1] - qa[k1 - 1])
        qb = np.minimum(qb, qa[k - 1])
        fpsa = psg * np.minimum(1.0, (psg - PSMIN) * rdps)
        fmass = tab["fm0"] * fpsa * np.minimum(5.0, qdif / (qmax - qb))
        cb = fmass
        fus, fuq, fds, fdq = fmass * se[k - 1], fmass * qmax, fmass * sb, fmass * qb
        dfse[k - 1] = np.where(conv, fds - fus, 0.0)
        dfqa[k - 1] = np.where(conv, fdq - fuq, 0.0)
        for k in range(kx - 1, 1, -1):
            act = conv & (k > itop)
            k1 = k - 1
            dse = fus - fds
            dqa_ = fuq - fdq
            enmass = E(k) * psg * cb
            fmass = np.where(act, fmass + enmass, fmass)
            fus = np.where(act, fus + enmass * se[k - 1], fus)
            fuq = np.where(act, fuq + enmass * qa[k - 1], fuq)
            sb = se[k1 - 1] + W(k1) * (se[k - 1] - se[k1 - 1])
            qb = qa[k1 - 1] + W(k1) * (qa[k - 1] - qa[k1 - 1])
            fds = np.where(act, fmass * sb, fds)
            fdq = np.where(act, fmass * qb, fdq)
            dse = dse + fds - fus
            dqa_ = dqa_ + fdq - fuq
            delq = RHIL * qsat[k - 1] - qa[k - 1]
            sec = act & (delq > 0.0)
            margin = np.where(act, np.minimum(margin, _margin(RHIL * qsat[k - 1], qa[k - 1])), margin)
            sec_flux |= sec
            fsq = SMF * cb * delq
            dqa_ = np.where(sec, dqa_ + fsq, dqa_)
            dfqa[kx - 1] = np.where(sec, dfqa[kx - 1] - fsq, dfqa[kx - 1])
            dfse[k - 1] = np.where(act, dse, dfse[k - 1])
            dfqa[k - 1] = np.where(act, dqa_, dfqa[k - 1])
        cbmf = np.where(conv, cb, 0.0)
        for k in range(3, kx - 2):                               # top layer k = itop (3 <= itop <= kx-3)
            top = conv & (itop == k)
            qsatb = qsat[k - 1] + W(k) * (qsat[k] - qsat[k - 1])
            pr = np.maximum(fuq - fmass * qsatb, 0.0)
            precnv = np.where(top, pr, precnv)
            dfse[k - 1] = np.where(top, fus - fds + ALHC * pr, dfse[k - 1])
            dfqa[k - 1] = np.where(top, fuq - fdq - pr, dfqa[k - 1])

    tt_cnv, qt_cnv = dfse.copy(), dfqa.copy()
    for k in range(2, kx + 1):                                   # physics.f90:124-127
        tt_cnv[k - 1] = tt_cnv[k - 1] * rps * tab["grdscp"][k - 1]
        qt_cnv[k - 1] = qt_cnv[k - 1] * rps * tab["grdsig"][k - 1]
    icnv = kx - itop

    # large-scale condensation (large_scale_condensation.f90:32-83)
    rtlsc = 1.0 / (TRLSC * 3600.0)
    tfact = ALHC / CP
    prg = P0 / GRAV
    tt_lsc = np.zeros((kx, n))
    qt_lsc = np.zeros((kx, n))
    psa2 = psg * psg
    lsc_top = np.zeros(n, bool)
    lsc_in = np.zeros(n, bool)
    for k in range(2, kx + 1):
        sig2 = fsg[k - 1] * fsg[k - 1]
        rhref = RHLSC + DRHLSC * (sig2 - 1.0)
        if k == kx:
            rhref = max(rhref, RHBLSC)
        dqmax = 10.0 * sig2 * rtlsc
        dqa = rhref * qsat[k - 1] - qa[k - 1]
        c = dqa < 0.0
        margin = np.minimum(margin, _margin(rhref * qsat[k - 1], qa[k - 1]))
        itop = np.where(c, np.minimum(k, itop), itop)
        dq = np.where(c, dqa * rtlsc, 0.0)
        qt_lsc[k - 1] = dq
        tt_lsc[k - 1] = np.where(c, tfact * np.minimum(-dq, dqmax * psa2), 0.0)
        if k == kx:
            lsc_top |= c
        else:
            lsc_in |= c
    precls = np.zeros(n)
    for k in range(2, kx + 1):
        precls = precls - dhs[k - 1] * prg * qt_lsc[k - 1]
    precls = precls * psg

    out = {"ttend": ttend + tt_cnv + tt_lsc, "qtend": qtend + qt_cnv + qt_lsc, "precnv": precnv, "precls": precls, "cbmf": cbmf,
           "iptop": itop.astype(np.int32), "icnv": icnv.astype(np.int32), "qsat": qsat, "rh": rh, "se": se, "margin": margin}
    # per branch: the columns that take it (branch_cols) and how many they are (branch)
    cols = {"psmin_cut": ~live, "conv_ktop2": via2, "conv_lqthr": via_q, "no_conv": ~conv, "secondary_flux": sec_flux,
            "lsc_kx": lsc_top, "lsc_interior": lsc_in, "qsat_warm": np.any(warm, axis=0), "qsat_cold": np.any(~warm, axis=0),
            "q_clamp": clamped}
    out["branch_cols"] = cols
    out["branch"] = dict({k: int(np.sum(v)) for k, v in cols.items()}, columns=int(n))
    return out


def block(tab, tg, qg, phig, pslg, ttend, qtend):
    """column_block on grids: tg, qg, phig, ttend, qtend [..., kx, il, ix], pslg [..., il, ix]; outputs shaped alike."""
    tg = np.asarray(tg, np.float64)
    kx = tg.shape[-3]
    lead, g2 = tg.shape[:-3], tg.shape[-2:]
    ncol = int(np.prod(lead, dtype=np.int64)) * g2[0] * g2[1]

    def cols(a):      # [..., kx, il, ix] -> [kx, ncol]
        return np.moveaxis(np.asarray(a, np.float64).reshape((-1, kx) + g2), 1, 0).reshape(kx, ncol)

    def grids(a):
        return np.moveaxis(a.reshape((kx, -1) + g2), 0, 1).reshape(lead + (kx,) + g2)
    r = column_block(tab, cols(tg), cols(qg), cols(phig), np.asarray(pslg, np.float64).reshape(ncol), cols(ttend), cols(qtend))
    out = {}
    for k, v in r.items():
        if isinstance(v, dict):          # branch counts / per-branch column masks (over the flattened columns)
            out[k] = v
        elif v.ndim == 2:
            out[k] = grids(v)
        else:
            out[k] = v.reshape(lead + g2)
    return out


# ---------------------------------------------------------------------------------------------------- seeded inputs
def _draw(kx, fsg, ncol, seed):
    """One draw of ncol physically shaped columns, [kx, ncol] (pslg [ncol]); seed selects the splitmix64 stream."""
    u = synth.splitmix64(seed, ncol * (3 * kx + 6)).reshape(3 * kx + 6, ncol)
    psa = 0.7 + 0.35 * u[0]                                     # ps/p0 in [0.7, 1.05): some columns below psmin
    sig = fsg[:, None]
    # T = 288 sigma^0.19, a surface anomaly of +-16 K that decays upwards, +-2 K per level: some columns below 273.16 K
    tg = 288.0 * sig ** 0.19 + (32.0 * u[1] - 16.0) * sig ** 3 + (4.0 * u[6:6 + kx] - 2.0)
    # relative humidity 0.2 .. 1.1 per level; a moist boundary layer in half of the columns (convection through either path)
    rh = 0.2 + 0.9 * u[6 + kx:6 + 2 * kx]
    moist = u[2] < 0.5
    rh[-2:] = np.where(moist, 0.85 + 0.25 * u[6 + kx:6 + kx + 2], rh[-2:])
    qg = rh * get_qsat(tg, psa, sig)
    neg = u[3] < 0.03                                           # a few slightly negative humidities (the clamp)
    qg[0] = np.where(neg, -1e-3 * u[4], qg[0])
    # hydrostatic geopotential from the surface up, plus a surface geopotential of 0 .. 1500 m
    rgas = f32(2.0 / 7.0) * CP
    phig = np.empty_like(tg)
    phig[-1] = GRAV * 1500.0 * u[5] ** 2 - rgas * tg[-1] * np.log(sig[-1, 0])
    for k in range(kx - 2, -1, -1):
        phig[k] = phig[k + 1] + 0.5 * rgas * (tg[k] + tg[k + 1]) * np.log(fsg[k + 1] / fsg[k])
    ttend = 1e-4 * (2.0 * u[6 + 2 * kx:6 + 3 * kx] - 1.0)
    qtend = 1e-7 * (2.0 * u[6 + 2 * kx:6 + 3 * kx][::-1] - 1.0)
    return tg, qg, phig, np.log(psa), ttend, qtend


MIN_MARGIN = 1e-9


def columns(tab, ncol, seed):
    """ncol physically shaped columns [kx, ncol] (pslg [ncol]): a column whose smallest decision margin (column_block) is below
    MIN_MARGIN is drawn again from the next stream.  Returns (tg, qg, phig, pslg, ttend, qtend)."""
    kx = tab["kx"]
    arrs = list(_draw(kx, tab["fsg"], ncol, seed))
    for attempt in range(1, 50):
        r = column_block(tab, *arrs)
        bad = np.nonzero(r["margin"] < MIN_MARGIN)[0]
        if bad.size == 0:
            return tuple(arrs)
        new = _draw(kx, tab["fsg"], ncol, seed + 7919 * attempt)
        for a, b in zip(arrs, new):
            a[..., bad] = b[..., bad]
    raise RuntimeError("could not draw columns clear of ties")


def grid_inputs(tab, shape, seed):
    """columns() laid out as nb states of grids: shape = (nb, il, ix) -> tg, qg, phig, ttend, qtend [nb, kx, il, ix], pslg [nb, il, ix]."""
    nb, il, ix = shape
    kx = tab["kx"]
    c = columns(tab, nb * il * ix, seed)
    g = [np.ascontiguousarray(np.moveaxis(a.reshape(kx, nb, il, ix), 0, 1)) for a in (c[0], c[1], c[2])]
    t = [np.ascontiguousarray(np.moveaxis(a.reshape(kx, nb, il, ix), 0, 1)) for a in (c[4], c[5])]
    return g[0], g[1], g[2], c[3].reshape(nb, il, ix), t[0], t[1]


# ---------------------------------------------------------------------------------------------------- model state + hook
def state(o, sp_trunc_state, seed):
    """dynstep.state with t, tr (q) and ps of BOTH time levels replaced by the spectra of physically shaped columns (grid_to_spec
    on the oracle `o`), so that the moist block takes every branch inside a time step."""
    st = dict(sp_trunc_state)
    tab = tables(o.table("hsg"))
    kx = tab["kx"]
    for j in range(2):
        tg, qg, phig, pslg, _, _ = grid_inputs(tab, (1, o.il, o.ix), seed + 31 * j)
        st["t"] = np.array(st["t"], copy=True)
        st["tr"] = np.array(st["tr"], copy=True)
        st["ps"] = np.array(st["ps"], copy=True)
        for k in range(kx):
            st["t"][j, k] = o.grid_to_spec(tg[0, k])
            st["tr"][j, k] = o.grid_to_spec(qg[0, k])
        st["ps"][j] = o.grid_to_spec(pslg[0])
    return st


def make_hook(record=None):
    """physics= hook of dynstep.oracle_dynamics_step: the moist block on time level 1 (tendencies.f90:203-204) through the oracle's
    spec_to_grid, ttend / qtend (= trtend of tracer 1) updated in place.  record (dict) receives the block's outputs."""
    def hook(o, st, ut, vt, tt, qt):
        kx = o.kx
        tab = tables(o.table("hsg"))
        phi = o.geopotential(st["t"][0], st["phis"])
        tg = np.stack([o.spec_to_grid(st["t"][0, k], 1) for k in range(kx)])
        qg = np.stack([o.spec_to_grid(st["tr"][0, k], 1) for k in range(kx)])
        phig = np.stack([o.spec_to_grid(phi[k], 1) for k in range(kx)])
        pslg = o.spec_to_grid(st["ps"][0], 1)
        r = block(tab, tg, qg, phig, pslg, tt, qt)
        tt[...] = r["ttend"]
        qt[...] = r["qtend"]
        if record is not None:
            record.update(r)
            record["grids"] = (tg, qg, phig, pslg)
    return hook
