"""An ensemble of E model states that goes through ONE time step's launches (include/spdy.h, "ensemble time step").

The layout is the single-state layout with every level dimension kx widened to E*kx, member-major inside it:

    vor, div, t, tr   complex128 (2, E, kx, nx, mx)      time level lv of all members = one contiguous stack of E*kx fields
    ps                complex128 (2, E, nx, mx)
    phis, tcorh, qcorh           (nx, mx)                shared by all members
    qcorh with member_qcorh      (E, nx, mx)             a field per member: what a coupled ensemble needs, since qcorh is made
                                                         from the member's own land and sea temperatures (SurfaceModel.forcing_dev)
    phi, phim                    (E, kx, nx, mx)         the step's geopotential, the physics' (time level 1)
    ug, vg                       (E, kx, il, ix)
    plain_g                      (4, E, kx, il, ix)      vorg | divg | tg | trg
    px, py                       (E, il, ix)
    U, V                         (3, E, kx, il, ix)      group-major operands of the direct batch: utend | -u T' | -u q
    PL                           (3 E kx + E, il, ix)    KE | ttend | qtend (E*kx each), then the E level-free fields
    pvor, pdiv / pspec           like U, V / PL, complex (nx, mx) fields

so the transforms are the existing calls with larger counts, the physics tendencies of all members are the first E*kx fields of
U, V and the second and third group of PL (states back to back at stride kx, what the column chain takes as nb = E), and member e of
the two column kernels works on level slot e*kx + k with group stride E*kx.

One step of a coupled ensemble, with a SurfaceModel and a Diagnostics of nmem = E: on a day's first step
model.forcing_dev(ens.qcorh); ens.step with the model's boundary() as bnd / albsfc and hfluxn, shf, evap, ssrd in "out";
guard.check_dev on time level 2 (ens.vor[1], ens.div[1], ens.t[1]); the host's newdate, and set_date when the day changed;
model.couple_dev(day, hfluxn, shf, evap, ssrd).

`step` is step(j1, j2, dt) of time_stepping.f90:35-121 and `startup` first_step of :12-24.  `output` gives every member's float32
snapshot (input_output.f90:184-206) and the ensemble mean and spread from one call (include/spdy.h, "ensemble output").  SPPT:
physics["sppt"], a Sppt with one pattern per member, is advanced and applied by `step` (include/spdy.h, "SPPT").  `analyse` is the
LETKF update of time level 1 from a Letkf's observations (include/spdy.h, "ensemble analysis"), `verify` its scores against a
Nature's truth (include/spdy.h, "nature run").  Not covered: the level-sharded
step."""
import numpy as np

from .spectral import MAX_PLEV

PROG = ("vor", "div", "t", "tr", "ps")
SHARED = ("phis", "tcorh", "qcorh")
ROB, WIL = float(np.float32(0.05)), float(np.float32(0.53))          # params.f90:32-33 (float32 literals widened)
SDRAG = 1.0 / (float(np.float32(24.0 * 30.0)) * 3600.0)              # time_stepping.f90:77, dynamical_constants.f90:22


def shapes(nmem, kx, nx, mx, il, ix, member_qcorh=False):
    """name -> (shape, is complex) of every array of an E-member ensemble (no device needed)"""
    E, s, g = nmem, (nx, mx), (il, ix)
    out = {n: ((2, E, kx) + s, True) for n in ("vor", "div", "t", "tr")}
    out["ps"] = ((2, E) + s, True)
    out.update({n: (s, True) for n in SHARED})
    if member_qcorh:
        out["qcorh"] = ((E,) + s, True)
    out.update(phi=((E, kx) + s, True), phim=((E, kx) + s, True))
    out.update(ug=((E, kx) + g, False), vg=((E, kx) + g, False), plain_g=((4, E, kx) + g, False), px=((E,) + g, False),
               py=((E,) + g, False))
    out.update(U=((3, E, kx) + g, False), V=((3, E, kx) + g, False), PL=((3 * E * kx + E,) + g, False))
    out.update(pvor=((3, E, kx) + s, True), pdiv=((3, E, kx) + s, True), pspec=((3 * E * kx + E,) + s, True))
    return out


class Ensemble:
    """The prognostics and the step's scratch of E members on the device, per-member views of them, and the step."""

    def __init__(self, sp, nmem, device="cuda", sdrag=SDRAG, rob=ROB, wil=WIL, arrays=None, member_qcorh=False):
        """member_qcorh: qcorh is (E, nx, mx), a humidity correction per member (the plan option "ens_member_qcorh", set by step).
        arrays: optionally {name: tensor} of caller-made contiguous tensors on `device` to use for those arrays in place of fresh
        ones, each of the shape and type `shapes` gives (a host that places the ensemble inside its own allocations)."""
        import torch
        if nmem < 1:
            raise ValueError("an ensemble has at least one member")
        need = nmem * max(3 * sp.kx + 1, 4 * sp.kx)      # the direct batch's plain fields; the inverse batch's (vorg | divg | tg | trg)
        if sp.max_batch < need:
            raise ValueError("the plan's max_batch must be >= nmem*max(3*kx+1, 4*kx) = %d" % need)
        self.sp, self.nmem, self.kx = sp, nmem, sp.kx
        self.sdrag, self.rob, self.wil, self.member_qcorh = sdrag, rob, wil, bool(member_qcorh)
        given = dict(arrays or {})
        for n, (shape, cplx) in shapes(nmem, sp.kx, sp.nx, sp.mx, sp.il, sp.ix, self.member_qcorh).items():
            dtype = torch.complex128 if cplx else torch.float64
            a = given.pop(n, None)
            if a is None:
                a = torch.zeros(shape, dtype=dtype, device=device)
            elif tuple(a.shape) != shape or a.dtype != dtype or not a.is_contiguous():
                raise ValueError("array %s must be a contiguous tensor of shape %s and type %s" % (n, shape, dtype))
            setattr(self, n, a)
        if given:
            raise ValueError("not arrays of an ensemble: %s" % sorted(given))
        E, kx, g = nmem, sp.kx, self.plain_g
        self.vorg, self.divg, self.tg, self.trg = g[0], g[1], g[2], g[3]
        self.PLg = self.PL[:3 * E * kx].view(3, E, kx, sp.il, sp.ix)             # the three level groups of PL ...
        self.PLs = self.PL[3 * E * kx:]                                          # ... and the E level-free fields
        # the physics tendencies of all members (tendencies.f90:203-206): (E, kx) grids each
        self.utend, self.vtend, self.ttend, self.qtend = self.U[0], self.V[0], self.PLg[1], self.PLg[2]

    # ------------------------------------------------------------------ views
    def member(self, e):
        """the single-state dict of views of member e: vor, div, t, tr (2, kx, nx, mx), ps (2, nx, mx) and the shared phis, tcorh,
        qcorh (with member_qcorh: the member's own qcorh).  A time level of a member, D[n][lv], is contiguous; the two time levels
        are E*kx (ps: E) fields apart."""
        D = {n: getattr(self, n)[:, e] for n in PROG}
        D.update({n: getattr(self, n) for n in SHARED})
        if self.member_qcorh:
            D["qcorh"] = self.qcorh[e]
        return D

    def set_member(self, e, st):
        """member e's prognostics from a single-state dict of host arrays (vor .. tr (2, kx, nx, mx), ps (2, nx, mx))"""
        import torch
        for n in PROG:
            getattr(self, n)[:, e].copy_(torch.as_tensor(np.ascontiguousarray(st[n], np.complex128)))

    def set_shared(self, st):
        """phis, tcorh and qcorh from host arrays; with member_qcorh, st["qcorh"] (nx, mx) goes to every member"""
        import torch
        for n in SHARED:
            getattr(self, n).copy_(torch.as_tensor(np.ascontiguousarray(st[n], np.complex128)))

    # ------------------------------------------------------------------ the step
    def physics_workspace(self, sppt=False):
        """before a capture that contains a step with physics; sppt: for a step whose physics has "sppt" """
        if sppt:
            self.sp.ens_physics_sppt_workspace(self.nmem)
        else:
            self.sp.ens_physics_workspace(self.nmem)

    def step(self, j1, j2, dt, physics=None, eps=None):
        """step(j1, j2, dt) for every member.  The dynamics read time level j2 (tendencies.f90:89-107), the physics time level 1
        (physics.f90:94-104).  physics: None (adiabatic) or a dict with "sw" (compute the shortwave on this step), "bnd" (dict of
        SFC_BOUNDARY fields, (E, il, ix) each), "albsfc" (E, il, ix), "rad" (E radiation states back to back) and optionally "out"
        (spdy_column_physics_out as a dict, every field E states long) and "sppt" (a Sppt of this plan with nmem == E: it is
        advanced, all members in three launches, and each member's pattern multiplies the physics' part of its tendencies; the
        reference advances once per physics call, the start-up steps included).  eps: the Robert filter's coefficient; by
        default the reference's, 0 when j1 == 1 and rob otherwise (time_stepping.f90:108-112)."""
        sp, E, kx, lv = self.sp, self.nmem, self.kx, j2 - 1
        eps = (0.0 if j1 == 1 else self.rob) if eps is None else eps
        flat = lambda a: a.view((-1,) + tuple(a.shape[-2:]))
        vor, div, t, tr = (flat(getattr(self, n)[lv]) for n in ("vor", "div", "t", "tr"))
        # everything that goes to the grid as one call: E*kx pairs, four plain segments of E*kx, E gradient fields
        sp.inverse_batch_segs_dev(vor, div, flat(self.ug), flat(self.vg), [vor, div, t, tr], flat(self.plain_g), self.ps[lv], self.px,
                                  self.py, kcos_pairs=2, kcos=1)
        sp.ens_grid_tendencies_dev(E, self.ug, self.vg, self.tg, self.vorg, self.divg, self.trg, self.px, self.py, self.U, self.V,
                                   self.PL)
        if physics is not None:
            sp.ens_geopotential_dev(E, self.t[0], self.phis, self.phim)
            args = (physics["sw"], self.vor[0], self.div[0], self.t[0], self.tr[0], self.phim, self.ps[0], physics["bnd"],
                    physics["albsfc"], physics["rad"], self.utend, self.vtend, self.ttend, self.qtend, physics.get("out"))
            pat = physics.get("sppt")
            if pat is None:
                sp.ens_physics_dev(E, *args)
            else:
                if pat.nmem != E:
                    raise ValueError("physics[\"sppt\"] must hold one pattern per member")
                pat.advance_dev()
                sp.ens_physics_sppt_dev(E, pat, *args)
        sp.set_option("ens_member_qcorh", 1 if self.member_qcorh else 0)      # read when the call below is enqueued
        sp.ens_direct_batch_spectral_step_dev(E, self.U, self.V, self.PL, self.pvor, self.pdiv, self.pspec, self.vor, self.div, self.t,
                                              self.tr, self.ps, self.phis, self.tcorh, self.qcorh, self.sdrag, j1, dt, eps, self.wil,
                                              self.phi, kcos=2)

    # ------------------------------------------------------------------ output
    def output_workspace(self):
        """before a capture that contains output"""
        self.sp.ens_output_workspace(self.nmem)

    def output_shapes(self):
        """group -> {field: shape} of what output returns (float32)"""
        E, kx, g = self.nmem, self.kx, (self.sp.il, self.sp.ix)
        lev = lambda lead: dict({n: lead + (kx,) + g for n in ("u", "v", "t", "q", "phi")}, ps=lead + g)
        return {"members": lev((E,)), "mean": lev(()), "spread": lev(())}

    def output(self, members=True, stats=True, use=None, phi=None, out=None):
        """The snapshot of every member and the ensemble statistics from time level 1, one call (input_output.f90:184-206 per member):
        {"members": {u, v, t, q, phi (E, kx, il, ix), ps (E, il, ix)}, "mean": {.. (kx, il, ix), ps (il, ix)}, "spread": {..}} of
        float32 device tensors; without `members` / `stats` the group(s) are left out.  mean = sum / n and spread = the sample
        standard deviation (n - 1) over the n members in use, formed in FP64; n = 1 gives spread 0, n = 0 NaN.
        use: None (all members), or a sequence or an int32 device tensor of E entries, non-zero = the member enters the statistics
        (the member fields are written for every member).  From a guard of the ensemble, once per output interval (its one
        synchronisation): use = [s == -1 for s in guard.stopped()] -- members the guard has not stopped have -1.
        phi: the geopotential of time level 1, (E, kx, nx, mx); by default self.phi.
        out: {group: {field: tensor}} of caller-made float32 tensors of output_shapes() to write into; inside a capture pass `out`
        and `use` as device tensors, after output_workspace(): the call then allocates nothing."""
        import torch
        if not members and not stats:
            raise ValueError("output: neither members nor stats wanted")
        dev = self.vor.device
        if use is not None and not torch.is_tensor(use):
            use = torch.tensor([1 if u else 0 for u in use], dtype=torch.int32, device=dev)
        if use is not None and (use.dtype != torch.int32 or use.numel() != self.nmem or not use.is_contiguous()):
            raise ValueError("use must be %d contiguous int32 entries" % self.nmem)
        res = {}
        for grp, shp in self.output_shapes().items():
            if not (members if grp == "members" else stats):
                continue
            given = (out or {}).get(grp)
            if given is None:
                given = {n: torch.empty(sh, dtype=torch.float32, device=dev) for n, sh in shp.items()}
            for n, sh in shp.items():
                a = given[n]
                if tuple(a.shape) != sh or a.dtype != torch.float32 or not a.is_contiguous():
                    raise ValueError("out[%s][%s] must be a contiguous float32 tensor of shape %s" % (grp, n, sh))
            res[grp] = given
        self.sp.ens_output_batch_dev(self.nmem, self.vor[0], self.div[0], self.t[0], self.tr[0], self.phi if phi is None else phi,
                                     self.ps[0], res.get("members"), res.get("mean"), res.get("spread"), use)
        return res

    def output_pressure_shapes(self, nlev):
        """group -> {field: shape} of what output_pressure returns for nlev pressure levels (float32); "below" -> its shape"""
        E, g = self.nmem, (self.sp.il, self.sp.ix)
        lev = lambda lead: dict({n: lead + (int(nlev),) + g for n in ("u", "v", "t", "q", "phi")}, ps=lead + g)
        return {"members": lev((E,)), "mean": lev(()), "spread": lev(()), "below": (int(nlev),) + g}

    def output_pressure(self, plev, coord="p", members=True, stats=True, use=None, phi=None, below=False, out=None):
        """output() on pressure levels (include/spdy.h, "pressure-level output"): every member's u, v, t, q, phi interpolated in the
        vertical to the pressures plev (Pa, a host sequence of 1 .. 32 levels in any order) by np.interp's rule -- coord "p": linear
        in p, what the reference's scripts/sigma_to_pressure.py does; "logp": linear in ln p -- and the mean and spread of the
        INTERPOLATED values over the members in use.  A level outside a member's column gets that member's end level's value.
        -> {"members": {u .. phi (E, nlev, il, ix), ps (E, il, ix)}, "mean": {.. (nlev, il, ix), ps (il, ix)}, "spread": {..},
        "below": (nlev, il, ix)} of float32 device tensors; without `members` / `stats` / `below` the entries are left out.  below:
        the number of members in use whose lowest model level lies above the level (the value there is the clamped one): the mask.
        members, stats, use, phi, out: as output(), out with the shapes of output_pressure_shapes(nlev) and "below" a tensor.  plev
        is read by this call: a captured call keeps its values."""
        import torch
        if not members and not stats:
            raise ValueError("output_pressure: neither members nor stats wanted")
        dev = self.vor.device
        if use is not None and not torch.is_tensor(use):
            use = torch.tensor([1 if u else 0 for u in use], dtype=torch.int32, device=dev)
        if use is not None and (use.dtype != torch.int32 or use.numel() != self.nmem or not use.is_contiguous()):
            raise ValueError("use must be %d contiguous int32 entries" % self.nmem)
        nlev = int(np.atleast_1d(plev).size)
        if not 1 <= nlev <= MAX_PLEV:
            raise ValueError("output_pressure: %d levels, not 1 .. %d" % (nlev, MAX_PLEV))
        res, shapes = {}, self.output_pressure_shapes(nlev)
        fits = lambda a, sh: tuple(a.shape) == sh and a.dtype == torch.float32 and a.is_contiguous()
        for grp in ("members", "mean", "spread"):
            if not (members if grp == "members" else stats):
                continue
            given = (out or {}).get(grp)
            if given is None:
                given = {n: torch.empty(sh, dtype=torch.float32, device=dev) for n, sh in shapes[grp].items()}
            for n, sh in shapes[grp].items():
                if not fits(given[n], sh):
                    raise ValueError("out[%s][%s] must be a contiguous float32 tensor of shape %s" % (grp, n, sh))
            res[grp] = given
        if below:
            res["below"] = (out or {}).get("below")
            if res["below"] is None:
                res["below"] = torch.empty(shapes["below"], dtype=torch.float32, device=dev)
            if not fits(res["below"], shapes["below"]):
                raise ValueError("out[below] must be a contiguous float32 tensor of shape %s" % (shapes["below"],))
        self.sp.ens_output_pressure_dev(self.nmem, self.vor[0], self.div[0], self.t[0], self.tr[0], self.phi if phi is None else phi,
                                        self.ps[0], plev, coord, res.get("members"), res.get("mean"), res.get("spread"),
                                        res.get("below"), use)
        return res

    # ------------------------------------------------------------------ analysis
    def observe(self, letkf, slot):
        """Observes time slot `slot` of letkf's network on time level 1 as it stands now (include/spdy.h, "observations in time
        slots"): the analysis' inverse batch into letkf's grid workspace and one launch that keeps every member's H x_e of the
        slot's observations; nothing of the ensemble changes.  Capturable; an empty slot enqueues nothing.  After every slot has
        been observed during the forecast, analyse(letkf, slots=True) is the 4D-LETKF update."""
        if getattr(letkf, "sp", None) is not self.sp:
            raise ValueError("observe: the Letkf must belong to the ensemble's plan")
        if letkf.nmem != self.nmem:
            raise ValueError("observe: the Letkf holds %d members, the ensemble %d" % (letkf.nmem, self.nmem))
        letkf.observe_dev(slot, self.vor[0], self.div[0], self.t[0], self.tr[0], self.ps[0])

    def analyse(self, letkf, use=None, slots=False):
        """The LETKF update of time level 1 of every member, in place (include/spdy.h, "ensemble analysis"): five launches whatever
        E is (six once the direct batch is of streaming size), capturable.  letkf: a Letkf of this plan with nmem == E, its
        observations set.  Time level 2 and phi are stale afterwards: continue with startup(delt).  Members are coupled: every
        member analysed must be finite.
        use: None (all members), or as output()'s: a sequence or an int32 device tensor of E entries, non-zero = the member is
        analysed (include/spdy.h, "member mask"; guard.use_dev() gives the guard's on the device).  The n members in use get, bit
        for bit, what an n-member Ensemble and Letkf give them; a member not in use is read into nothing shared and keeps every
        bit of its state; n < 2 leaves the whole state.  One launch more.  The tensor is read when the kernels run: a captured
        analysis follows its contents.
        slots=True: the slot analysis (include/spdy.h, "observations in time slots"): H x_e of every observation is what
        observe(letkf, s) kept at its slot's time, the increments are formed on the state as it stands now; the same launches."""
        if getattr(letkf, "sp", None) is not self.sp:
            raise ValueError("analyse: the Letkf must belong to the ensemble's plan")
        if letkf.nmem != self.nmem:
            raise ValueError("analyse: the Letkf holds %d members, the ensemble %d" % (letkf.nmem, self.nmem))
        letkf.analyse_dev(self.vor[0], self.div[0], self.t[0], self.tr[0], self.ps[0], use, slots)

    def obs_stats(self, letkf, slot, use=None):
        """The stats-only call on time level 1 as it stands now (include/spdy.h, "background check and observation statistics"):
        the analysis' inverse batch and observation stage, then the statistics of row `slot` over the used set of letkf's latest
        checked analysis, with that analysis' departure as dep_b -- after analyse(letkf) this is observation-minus-analysis, and
        sum_dep_depb the Desroziers product.  Nothing of the ensemble changes; capturable.  letkf.obs_stats(slot) downloads the row."""
        if getattr(letkf, "sp", None) is not self.sp:
            raise ValueError("obs_stats: the Letkf must belong to the ensemble's plan")
        if letkf.nmem != self.nmem:
            raise ValueError("obs_stats: the Letkf holds %d members, the ensemble %d" % (letkf.nmem, self.nmem))
        letkf.stats_dev(slot, self.vor[0], self.div[0], self.t[0], self.tr[0], self.ps[0], use)

    def verify(self, letkf, nature, slot=0, use=None):
        """The scores of time level 1 against a Nature's truth (include/spdy.h, "nature run"): rmse and bias of the ensemble mean and
        the spread, per variable and level, into nature.scores(slot).  Three launches, capturable; nothing of the ensemble changes.
        letkf: a Letkf of this plan with nmem == E, whose grid workspace the call uses; nature: a Nature of this plan.  use: as
        analyse's: the scores over the members in use."""
        if getattr(letkf, "sp", None) is not self.sp or getattr(nature, "sp", None) is not self.sp:
            raise ValueError("verify: the Letkf and the Nature must belong to the ensemble's plan")
        if letkf.nmem != self.nmem:
            raise ValueError("verify: the Letkf holds %d members, the ensemble %d" % (letkf.nmem, self.nmem))
        nature.verify(letkf, self.vor[0], self.div[0], self.t[0], self.tr[0], self.ps[0], slot, use)

    def startup(self, delt, physics=None):
        """first_step (time_stepping.f90:12-24): the forward half step, the first leapfrog step and the three initialize_implicit
        calls.  physics: None, or a function n -> the physics dict of step n (n = -1, 0 number the two steps)."""
        sp = self.sp
        phys = (lambda n: None) if physics is None else physics
        sp.initialize_implicit(0.5 * delt)
        self.step(1, 1, 0.5 * delt, phys(-1))
        sp.synchronize()
        sp.initialize_implicit(delt)
        self.step(1, 2, delt, phys(0))
        sp.synchronize()
        sp.initialize_implicit(2.0 * delt)
