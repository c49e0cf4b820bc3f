"""The ensemble analysis on the device (spdy_letkf_* in include/spdy.h, "ensemble analysis").

A Letkf belongs to a plan and an ensemble size.  One analysis: set_obs(...), then Ensemble.analyse(letkf) on the spectral state
(five launches, six where the direct batch is of streaming size; in place, time level 1) or analyse_grid(...) on a gridded
ensemble; fields() gives the observation-space quantities of that call, so observation-minus-background statistics need no
second operator.  weight_stride=(si, sj) solves the local problems on every si-th longitude and sj-th row only and gives the
other columns the bilinear interpolation of those columns' transforms (one launch more); (1, 1), the default, solves every column.
set_obs(..., p=...) takes observations of u, v, t or q given at a pressure (lev == OBS_AT_P): they are interpolated in the vertical
per member, linearly in ln p (include/spdy.h, "observations at a pressure").  After an analysis the run continues
with Ensemble.startup(delt): time level 2 and phi are stale until then.  Members are coupled, a non-finite member makes every
column it touches non-finite: pass use=, a member mask on the device (Diagnostics.use_dev gives the guard's), to analyse the
members the guard has not stopped and leave the others alone, bit for bit (include/spdy.h, "member mask").
set_relaxation(rtpp, rtps) relaxes the analysis towards the background where observations acted, one launch more (include/spdy.h,
"relaxation").  set_slots(first) divides the observations into time slots: Ensemble.observe(letkf, s) during the
forecast takes each member's H x_e at the slot's own time, Ensemble.analyse(letkf, slots=True) is then one update from all of them,
the 4D-LETKF (include/spdy.h, "observations in time slots").  set_background_check(gross) tests every departure
against spread plus error before the local analyses read it and keeps the counts and sums of an innovation table per group of
observations, one launch more; obs_stats() downloads them (include/spdy.h, "background check and observation statistics";
DESIGN.md s27).  set_adaptive_inflation() replaces the scalar rho by a field per level and column that every analysis reads
and then advances from its own innovation statistics, two launches more (include/spdy.h, "adaptive inflation")."""
import ctypes

import numpy as np

from ._lib import ERR_HIP, check
from .columns import DeviceField, PlanObject

OBS_U, OBS_V, OBS_T, OBS_Q, OBS_PS = range(5)
OBS_AT_P = -1                         # SPDY_OBS_AT_P: as lev, the observation sits at the pressure p
# host table -> (dtype, shape); -1: what the library's count leaves
_TABLES = {"stencil_index": (np.int64, (-1, 4)), "stencil_weight": (np.float64, (-1, 4)), "unit": (np.float64, (-1, 3)),
           "lnsigma": (np.float64, (-1,)), "rinv": (np.float64, (-1,)), "coarse_columns": (np.int64, (-1,)),
           "interp_index": (np.int64, (-1, 4)), "interp_weight": (np.float64, (-1, 4)), "lnp": (np.float64, (-1,)),
           "adaptive_inflation": (np.float64, (-1,)), "slot_first": (np.int64, (-1,))}
_PER_OBS, _PER_OBS_MEMBER = (lambda l: (l.nobs,)), (lambda l: (l.nobs, l.nmem))
# device field -> the shape of a Letkf's, all float64
_FIELDS = {"hx": _PER_OBS_MEMBER, "hxmean": _PER_OBS, "y": _PER_OBS_MEMBER, "departure": _PER_OBS,
           "weights": lambda l: (check(l.lib.spdy_letkf_table(l.h, b"coarse_columns", None, 0)), l.sp.kx, l.nmem, l.nmem),
           "value": _PER_OBS, "grid": lambda l: ((4 * l.sp.kx + 1) * l.nmem,) + l.sp.grid_shape,
           "obs_lnsigma": _PER_OBS, "obs_used": _PER_OBS, "members_used": lambda l: (1,),
           "inflation": lambda l: (4 * l.sp.kx + 1,) + l.sp.grid_shape, "obs_check": _PER_OBS, "obs_rinv": _PER_OBS,
           "obs_stats": lambda l: (QC_SLOTS, QC_MAX_GROUPS, len(QC_COLUMNS)),
           "rho": lambda l: (l.sp.kx,) + l.sp.grid_shape, "infl_parm": lambda l: (3, l.sp.kx) + l.sp.grid_shape, "obs_s2": _PER_OBS,
           "slot_ps": _PER_OBS_MEMBER, "slot_out": _PER_OBS_MEMBER}
LETKF_TABLES, LETKF_FIELDS = tuple(_TABLES), tuple(_FIELDS)
QC_MAX_GROUPS, QC_SLOTS = 64, 4       # SPDY_QC_MAX_GROUPS, SPDY_QC_SLOTS
# the ten numbers of a group's row of the statistics, in the header's order
QC_COLUMNS = ("n_all", "n_out", "n_rej", "n_used", "sum_dep", "sum_dep2", "sum_s2", "sum_err2", "sum_dep_depb", "sum_depb")


class Obs(ctypes.Structure):          # spdy_obs (include/spdy.h)
    _fields_ = [("var", ctypes.c_int), ("lev", ctypes.c_int), ("lon", ctypes.c_double), ("lat", ctypes.c_double),
                ("value", ctypes.c_double), ("error", ctypes.c_double)]


class PObs(ctypes.Structure):         # spdy_pobs (include/spdy.h)
    _fields_ = [("var", ctypes.c_int), ("lev", ctypes.c_int), ("p", ctypes.c_double), ("lon", ctypes.c_double),
                ("lat", ctypes.c_double), ("value", ctypes.c_double), ("error", ctypes.c_double)]


def use_mask(use, nmem, device):
    """`use` of a masked call as Ensemble.output takes it -> None (all members) or a contiguous int32 tensor of nmem entries on
    `device`: a sequence becomes one (non-zero / true = in use), a tensor is checked"""
    import torch
    if use is None:
        return None
    if not torch.is_tensor(use):
        use = list(use)
        if len(use) != nmem:
            raise ValueError("use must be %d contiguous int32 entries" % nmem)
        use = torch.tensor([1 if u else 0 for u in use], dtype=torch.int32, device=device)
    if use.dtype != torch.int32 or use.numel() != nmem or not use.is_contiguous():
        raise ValueError("use must be %d contiguous int32 entries" % nmem)
    return use


def _ptrs(tensors, use=False):
    """The device pointers of five or ten tensors as an entry point's arguments.  use: False, the entry point takes no member mask;
    otherwise its pointer goes last, NULL for None (all members)"""
    p = [ctypes.c_void_p(a.data_ptr()) for a in tensors]
    return p if use is False else p + [None if use is None else ctypes.c_void_p(use.data_ptr())]


class _DeviceView:
    """a DeviceField of float64 as the array interface torch.as_tensor wraps without a copy"""

    def __init__(self, f):
        self.__cuda_array_interface__ = {"shape": f.shape, "typestr": "<f8", "data": (f.ptr, False), "version": 2}


class Letkf(PlanObject):
    """sigma_h: horizontal localisation scale in metres; sigma_v: vertical scale in ln sigma (<= 0: none); rho: multiplicative
    inflation of the background covariance; weight_stride: set_weight_stride; rtpp, rtps: set_relaxation; gross, groups:
    set_background_check (groups needs observations, so here it must be None unless max_obs == 0); adaptive: False, True
    (set_adaptive_inflation with its defaults) or a dict of its arguments.  2 <= nmem <= 32; the plan needs
    max_batch >= nmem (2 kx + 1)."""
    PREFIX = "spdy_letkf"

    def __init__(self, sp, nmem, max_obs, sigma_h, sigma_v=0.0, rho=1.0, weight_stride=(1, 1), rtpp=0.0, rtps=0.0, gross=0.0,
                 groups=None, adaptive=False):
        self.sp, self.lib = sp, sp.lib
        if sp.device >= 0:
            sp._sync_stream()
        h = ctypes.c_void_p()
        check(self.lib.spdy_letkf_create(sp.h, int(nmem), int(max_obs), ctypes.byref(h)))
        self.h, self.nmem, self.max_obs, self.nobs = h, int(nmem), int(max_obs), 0
        self.slots = None
        self.weight_stride = (1, 1)
        self.set_localization(sigma_h, sigma_v, rho)
        if tuple(weight_stride) != (1, 1):
            self.set_weight_stride(*weight_stride)
        self.relaxation = (0.0, 0.0)
        if (rtpp, rtps) != (0.0, 0.0):
            self.set_relaxation(rtpp, rtps)
        self.gross, self.ngroups, self.stats_slot = 0.0, 5, 0
        if gross != 0.0 or groups is not None:
            self.set_background_check(gross, groups)
        self.adaptive = None
        if adaptive:
            self.set_adaptive_inflation(**(adaptive if isinstance(adaptive, dict) else {}))

    def _call(self, fn, *args, reset=None):
        """One call of the library on this object, after whatever the caller's torch stream holds (the plan's stream synchronised
        with it).  reset: the mirrored attributes as the library leaves the object where a setter's allocation or copy fails
        (SPDY_ERR_HIP), set before the error is raised"""
        if self.sp.device >= 0:
            self.sp._sync_stream()
        rc = fn(self.h, *args)
        if rc == ERR_HIP and reset:
            for name, value in reset.items():
                setattr(self, name, value)
        check(rc)

    def _analyse(self, plain, masked, slotted, tensors, use, slots):
        """the analysis entry point of the route: the slot call takes the mask or NULL, the plain call none"""
        if slots:
            self._call(slotted, *_ptrs(tensors, use))
        elif use is None:
            self._call(plain, *_ptrs(tensors))
        else:
            self._call(masked, *_ptrs(tensors, use))

    def set_adaptive_inflation(self, sigma_b=0.04, rho_min=0.9, rho_max=3.0, on=True):
        """Adaptive inflation (include/spdy.h, "adaptive inflation"): the analysis reads a field rho [kx, il, ix]
        in the scalar rho's place and every analysis call then advances it from its own innovation statistics, two launches more,
        last.  sigma_b (finite, >= 0): the standard deviation given to the prior rho, 0.04 as in Miyoshi (2011): with a few hundred
        effective observations the field moves a few per cent of the way to the observed value per analysis; 0 freezes the field.
        rho_min, rho_max (0 < rho_min <= rho_max): the estimate is a ratio of noisy sums, so it is kept in a range -- by default
        [0.9, 3.0]: a little deflation is allowed, since an estimate that may not go below 1 is biased upwards wherever the true
        value is 1, and 3.0 (1.7 in spread) bounds what a run of unrepresentative departures can do before the next analyses
        bring it back.  on=False: the scalar rho again; the field is kept.  The first on=True allocates the field, filled with the
        object's scalar rho: it synchronises the plan's stream and is not possible inside a capture; later settings only change
        the numbers, read when an analysis is enqueued.  self.adaptive: (sigma_b, rho_min, rho_max), or None while off."""
        self._call(self.lib.spdy_infl_set, 1 if on else 0, float(sigma_b), float(rho_min), float(rho_max),
                   reset={"adaptive": None})                 # the allocation failed: the object is left off
        self.adaptive = (float(sigma_b), float(rho_min), float(rho_max)) if on else None

    def fill_inflation(self, rho0):
        """The field rho set to rho0 (finite, > 0) everywhere (spdy_infl_fill); allocates it if need be and leaves adaptive
        inflation as it is, on or off.  Synchronises the plan's stream; not inside a capture."""
        self._call(self.lib.spdy_infl_fill, float(rho0))

    def inflation_field(self):
        """field("rho"): the inflation field [kx, il, ix] in the object's own memory, writable -- upload() sets any field, numpy()
        saves one for a restart.  Valid on every object of a device plan (asking makes the block; not inside a capture)."""
        return self.field("rho")

    def set_background_check(self, gross=0.0, groups=None, slot=0):
        """The background check and the observation statistics (include/spdy.h, "background check and observation statistics";
        DESIGN.md s27).  gross (finite, >= 0): an observation whose squared departure exceeds gross^2 (s2 + error^2), s2 the
        ensemble's variance at the observation, takes no part in the analysis (field("obs_check"): 0 passed, 1 rejected, 2 out of
        column; field("obs_used")); 0: nothing is rejected.  groups: None, the observation's variable (5 groups), or nobs integers
        in [0, max + 1) for the current observations, at most 64 groups -- the rows of obs_stats(); set_obs returns them to the
        default.  slot: which of the 4 rows of statistics the next calls fill, read when a call is enqueued.  (0, None), the
        default: off, the analysis is the one it always was; otherwise every analysis call has one launch more.  Synchronises the
        plan's stream; not inside a capture.  The first setting that turns anything on allocates a small block."""
        table, n = None, 0
        if groups is not None:
            g = np.atleast_1d(np.asarray(groups))
            if g.ndim != 1 or g.shape[0] != self.nobs or (g.size and not np.issubdtype(g.dtype, np.integer)):
                raise ValueError("set_background_check: groups must be %d integers, one per observation" % self.nobs)
            n = int(g.max()) + 1 if g.size else 1
            table = (ctypes.c_int * max(g.shape[0], 1))(*[int(v) for v in g])
        self._call(self.lib.spdy_qc_set, float(gross), n, None if table is None else ctypes.cast(table, ctypes.c_void_p),
                   reset={"gross": 0.0, "ngroups": 5})         # the object is left off
        self.gross, self.ngroups = float(gross), n if table is not None else 5
        check(self.lib.spdy_qc_set_slot(self.h, int(slot)))
        self.stats_slot = int(slot)

    def obs_stats(self, slot=None):
        """The statistics of a row (default: the current one) as the latest call that filled it left them: a dict of QC_COLUMNS,
        each an array of ngroups values -- the counts n_all, n_out, n_rej, n_used and, over the used observations, the sums of
        the departure, its square, s2, error^2, departure times the analysis call's departure, and that departure.  Downloads:
        synchronises the plan's stream."""
        slot = self.stats_slot if slot is None else int(slot)
        if not 0 <= slot < QC_SLOTS:
            raise ValueError("obs_stats: slot outside [0, %d)" % QC_SLOTS)
        rows = self.field("obs_stats").numpy()[slot, :self.ngroups]
        return {name: rows[:, i].copy() for i, name in enumerate(QC_COLUMNS)}

    def stats_grid(self, slot, ug, vg, tg, qg, psg, use=None):
        """The stats-only call on a gridded ensemble (spdy_qc_stats_grid_dev): the observation stage on these grids and the
        statistics of row `slot` with the used set and the departure of the latest checked analysis as dep_b; fields hx, hxmean, y
        and departure are overwritten, no state changes.  Two launches (three with use); capturable."""
        x = (ug, vg, tg, qg, psg)
        self._grids("stats_grid", x)
        self._call(self.lib.spdy_qc_stats_grid_dev, *_ptrs(x, use_mask(use, self.nmem, self._device())), int(slot))

    def stats_dev(self, slot, vor, div, t, q, ps, use=None):
        """spdy_qc_stats_dev: stats_grid on time level 1 of an ensemble's spectra (Ensemble.obs_stats)."""
        self._call(self.lib.spdy_qc_stats_dev, *_ptrs((vor, div, t, q, ps), use_mask(use, self.nmem, self._device())), int(slot))

    def set_relaxation(self, rtpp=0.0, rtps=0.0):
        """Relaxation of the analysis towards the background (include/spdy.h, "relaxation"), both in [0, 1]: rtpp
        relaxes the analysis perturbations to the background perturbations (1: only the mean moves), rtps then relaxes their
        spread to the background spread (1: the spread is restored).  Both are exactly 1 where the analysis changed nothing.
        (0, 0), the default: none, the analysis is the one it always was.  Read when an analysis is enqueued: a captured analysis
        keeps the values of its capture.  The first setting other than (0, 0) allocates a workspace of (4 kx + 1) nmem grids: it
        synchronises the plan's stream and is not possible inside a capture; later settings only change the two numbers."""
        self._call(self.lib.spdy_relax_set, float(rtpp), float(rtps),
                   reset={"relaxation": (0.0, 0.0)})          # the allocation failed: the object is left at (0, 0)
        self.relaxation = (float(rtpp), float(rtps))

    def set_localization(self, sigma_h, sigma_v=0.0, rho=1.0):
        """read when an analysis is enqueued: a captured analysis keeps the values of its capture"""
        check(self.lib.spdy_letkf_set_localization(self.h, float(sigma_h), float(sigma_v), float(rho)))

    def set_weight_stride(self, si, sj):
        """Weight interpolation: the local problems are solved at longitudes 0, si, 2 si, ... (si divides ix, si <= ix/2) and rows 0,
        sj, 2 sj, ... and il-1 (1 <= sj <= il-1); every other column gets the bilinear interpolation, in index space, of the
        transforms of the four coarse columns around it.  (1, 1): every column is solved, as without this call.  Builds and uploads
        the tables and allocates the weight buffer; synchronises the plan's stream; not inside a capture, and a graph captured
        before the call has to be captured again."""
        self._call(self.lib.spdy_letkf_set_weight_stride, int(si), int(sj),
                   reset={"weight_stride": (1, 1)})            # the object is left at stride (1, 1)
        self.weight_stride = (int(si), int(sj))

    def set_obs(self, var, lev, lon, lat, value, error, p=None):
        """The observations of the next analysis, arrays of one length (0 .. max_obs): var OBS_U .. OBS_PS, lev 0 .. kx-1 (ignored
        for OBS_PS), lon, lat in degrees, value and error in the model's units (q in g/kg, ps as log(p/p0)).  Every field is
        validated before anything changes.  Synchronises the plan's stream; not inside a capture.
        p (spdy_pobs_set; include/spdy.h, "observations at a pressure"): an array of pressures in Pa of the same length; an
        observation of u, v, t or q with lev == OBS_AT_P then sits at its p (finite, > 0) and is interpolated in the vertical,
        linearly in ln p, member by member; the others are as without p, their p is ignored.  An at-pressure observation that is
        above the top level or below the lowest one of any member at any of its four points takes no part in that analysis
        (field("obs_used")).  Without an at-pressure observation the object is left exactly as without p."""
        names = (var, lev, lon, lat, value, error) + (() if p is None else (p,))
        cols = [np.atleast_1d(np.asarray(a)) for a in names]
        n = cols[0].shape[0]
        if any(c.ndim != 1 or c.shape[0] != n for c in cols):
            raise ValueError("set_obs: var, lev, lon, lat, value, error%s must be one-dimensional arrays of one length"
                             % ("" if p is None else ", p"))
        if n > self.max_obs:
            raise ValueError("set_obs: %d observations, the object holds %d" % (n, self.max_obs))
        if p is None:
            obs = (Obs * max(n, 1))()
            for o in range(n):
                obs[o] = Obs(int(cols[0][o]), int(cols[1][o]), float(cols[2][o]), float(cols[3][o]), float(cols[4][o]), float(cols[5][o]))
            call = self.lib.spdy_letkf_set_obs
        else:
            obs = (PObs * max(n, 1))()
            for o in range(n):
                obs[o] = PObs(int(cols[0][o]), int(cols[1][o]), float(cols[6][o]), float(cols[2][o]), float(cols[3][o]),
                              float(cols[4][o]), float(cols[5][o]))
            call = self.lib.spdy_pobs_set
        self._call(call, n, ctypes.cast(obs, ctypes.c_void_p),
                   reset={"nobs": 0, "slots": None})           # a copy failed, the object holds no observations now
        self.nobs, self.slots, self.ngroups = n, None, 5

    def set_slots(self, first):
        """Divides the current observations into len(first) - 1 time slots (include/spdy.h, "observations in time slots"): slot s is
        the observations first[s] <= o < first[s+1]; first[0] == 0, non-decreasing, first[-1] == nobs, at most 32 slots, a slot may
        be empty.  None: no slots.  Host only: nothing is launched, allocated or synchronised, and it may be called at any time; the
        ranges are read when a call is enqueued, so a captured graph keeps those of its capture.  Every slot then counts as not
        observed.  set_obs returns the object to no slots.  self.slots: the ranges as a tuple, or None."""
        if first is None:
            check(self.lib.spdy_slot_set(self.h, 0, None))
            self.slots = None
            return
        f = np.atleast_1d(np.asarray(first))
        if f.ndim != 1 or f.shape[0] < 2 or not np.issubdtype(f.dtype, np.integer):
            raise ValueError("set_slots: first must be a one-dimensional array of nslots + 1 >= 2 integers")
        arr = (ctypes.c_int * f.shape[0])(*[int(v) for v in f])
        check(self.lib.spdy_slot_set(self.h, f.shape[0] - 1, ctypes.cast(arr, ctypes.c_void_p)))
        self.slots = tuple(int(v) for v in f)

    def _grids(self, what, x):
        """the five grids of an ensemble checked: ug .. qg [nmem, kx, il, ix], psg [nmem, il, ix] contiguous float64 tensors"""
        import torch
        sp, E = self.sp, self.nmem
        for a, s in zip(x, [(E, sp.kx) + sp.grid_shape] * 4 + [(E,) + sp.grid_shape]):
            if tuple(a.shape) != s or a.dtype != torch.float64 or not a.is_contiguous():
                raise ValueError("%s: expected a contiguous float64 tensor of shape %s, got %s" % (what, s, tuple(a.shape)))

    def observe_grid(self, slot, ug, vg, tg, qg, psg):
        """Observes time slot `slot` on a gridded ensemble (analyse_grid's layout): every member's H x_e of the slot's observations
        goes to its rows of field("hx") -- for a network with observations at a pressure also the members' ps at the stations and
        their out-of-column flags, field("slot_ps") and field("slot_out") -- and nothing else is written.  One launch, none for an
        empty slot; capturable; nothing synchronises.  The analysis with slots=True then uses these rows."""
        x = (ug, vg, tg, qg, psg)
        self._grids("observe_grid", x)
        self._call(self.lib.spdy_slot_observe_grid_dev, int(slot), *_ptrs(x))

    def observe_dev(self, slot, vor, div, t, q, ps):
        """spdy_slot_observe_dev: observe_grid on time level 1 of an ensemble's spectra (Ensemble.observe): the analysis' inverse batch
        into the grid workspace -- field("grid") then holds the gridded ensemble of that time -- and the slot's launch.  Nothing of
        the ensemble changes; capturable; an empty slot enqueues nothing."""
        self._call(self.lib.spdy_slot_observe_dev, int(slot), *_ptrs((vor, div, t, q, ps)))

    def table(self, name):
        """A host table of the current observations (LETKF_TABLES): stencil_index [nobs, 4] (grid points j*ix+i, int64),
        stencil_weight [nobs, 4], unit [nobs, 3], lnsigma [nobs] (ln(p/p0) for an observation at a pressure: its value at ps = 0),
        rinv [nobs], lnp [nobs] (ln(p/p0) of the observations at a pressure, 0 for the others; empty after a set_obs without p);
        or of the weight interpolation: coarse_columns
        [ncoarse] (grid columns j*ix+i, int64, ascending), interp_index [ncol, 4] (entries of coarse_columns, int64; an entry of
        weight zero repeats the first), interp_weight [ncol, 4]; all three are empty at stride (1, 1); or of the time slots:
        slot_first [nslots + 1] (int64), the ranges of set_slots, empty with no slots."""
        out = self._table(name)           # an unknown name is the library's to refuse
        dtype, shape = _TABLES[name]
        return out.astype(dtype, copy=False).reshape(shape)

    def field(self, name):
        """A device field of the latest analysis call (LETKF_FIELDS): hx, y [nobs, nmem], hxmean, departure [nobs]; a DeviceField
        in the object's own memory, the pointers never change.  weights [ncoarse, kx, nmem, nmem]: the transforms T[f][e] of the
        coarse columns, at a weight stride other than (1, 1) only; set_weight_stride moves it.  value [nobs]: the observation values
        the next analysis reads, as set_obs or Nature.observe wrote them (valid at once, not only after an analysis).  grid
        [(4 kx + 1) nmem, il, ix]: the grid workspace, u | v | t | q (nmem kx grids each, member-major) | ps (nmem) -- the gridded
        ensemble after Nature.verify, the increments after Ensemble.analyse.  obs_lnsigma [nobs]: ln sigma_o the latest analysis
        call localised with (for an observation at a pressure ln(p/p0) minus the ensemble-mean ps at its place, formed in that
        call); obs_used [nobs]: 1.0, or 0.0 for an at-pressure observation that was out of some member's column in that call.
        members_used [1]: the members the latest analysis call analysed, nmem without a mask; ask for it after the call -- it is
        one of two words, that of the kind of call (masked or not) enqueued last.  inflation [4 kx + 1, il, ix]: the factor f
        of every grid item (u | v | t | q at kx levels, then ps) in the latest analysis call with relaxation on, exactly 1.0 where
        the analysis changed nothing; zero until the first such call.  slot_ps, slot_out [nobs, nmem]: for a network with
        observations at a pressure, every member's ps at the station and its out-of-column flag (1.0 / 0.0) as observe_grid /
        observe_dev left them for the observation's slot (include/spdy.h, "observations in time slots"); otherwise not written.
        obs_check [nobs]: 0.0 passed, 1.0 rejected by the background check, 2.0 out of column, of the latest analysis call with the
        check on; obs_stats [4, 64, 10]: the statistics' table (obs_stats() names its columns); both zero until then (asking for
        one before set_background_check has made their block makes it: not inside a capture).  obs_rinv [nobs]: the per-call copy of 1/error^2 the local analyses read,
        exactly 0 for an observation that took no part; written by an analysis of a network with observations at a pressure or
        with the background check on.  rho [kx, il, ix]: the field of adaptive inflation, which the next analysis call reads
        and then advances (writable); infl_parm [3, kx, il, ix]: the sums p1, p2, p3 of the latest adaptive call; obs_s2 [nobs]: the
        ensemble variance at every observation in that call; all three are of one block that asking for any of them makes (not
        inside a capture), adaptive inflation stays off then."""
        p = ctypes.c_void_p()
        check(self.lib.spdy_letkf_field(self.h, name.encode(), ctypes.byref(p)))
        return DeviceField(self.sp, p.value, _FIELDS[name](self))

    def fields(self):
        """{"hx": [nobs, nmem], "hxmean": [nobs], "departure": [nobs]} of the latest analysis call: float64 device tensors that
        are views of the object's own memory (no copy; the next analysis call overwrites them, and they die with the object)."""
        import torch
        dev, out = "cuda:%d" % self.sp.device, {}
        for name in ("hx", "hxmean", "departure"):
            f = self.field(name)
            out[name] = torch.as_tensor(_DeviceView(f), device=dev) if self.nobs else torch.empty(f.shape, dtype=torch.float64, device=dev)
        return out

    def _device(self):
        return "cuda:%d" % self.sp.device if self.sp.device >= 0 else "cpu"

    def analyse_grid(self, ug, vg, tg, qg, psg, out=None, use=None, slots=False):
        """The increments (du, dv, dt, dq, dps) of a gridded ensemble: ug .. qg [nmem, kx, il, ix], psg [nmem, il, ix] float64
        device tensors; out: five tensors of those shapes to write into (they may be the inputs), by default fresh ones.
        Two launches, three at a weight stride other than (1, 1), one more with relaxation on (set_relaxation: the increments are
        then the relaxed ones, and field("inflation") holds their factors); capturable when `out` is given.
        use: None (all members), or a sequence or a contiguous int32 device tensor of nmem entries, non-zero = in use (include/spdy.h,
        "member mask"): the n members in use get the increments an n-member Letkf gives them, bit for bit, the others exactly 0.0
        and are not read into anything shared; n < 2: all zero.  One launch more; the tensor is read when the kernels run, so a
        captured call follows its contents.
        slots=True: the slot analysis (include/spdy.h, "observations in time slots") -- H x_e of every observation is what
        observe_grid / observe_dev left for its slot, the increments are formed on this ensemble; the same launches, with the kernel
        that finishes the observation-space quantities in the observation kernel's place.  Every non-empty slot must have been
        observed since set_slots."""
        import torch
        sp, E = self.sp, self.nmem
        use = use_mask(use, E, self._device())
        x = (ug, vg, tg, qg, psg)
        if out is None:
            out = tuple(torch.empty_like(a) for a in x)
        if len(out) != 5:
            raise ValueError("analyse_grid: out must hold five tensors")
        self._grids("analyse_grid", x)
        self._grids("analyse_grid", out)
        self._analyse(self.lib.spdy_letkf_analyse_grid_dev, self.lib.spdy_mask_letkf_analyse_grid_dev, self.lib.spdy_slot_analyse_grid_dev,
                      x + tuple(out), use, slots)
        return tuple(out)

    def analyse_dev(self, vor, div, t, q, ps, use=None, slots=False):
        """spdy_ens_letkf_dev: time level 1 of an ensemble, in place (Ensemble.analyse); use: as analyse_grid's, the members not in
        use keep every bit (spdy_mask_ens_letkf_dev).  With relaxation on (set_relaxation) the increments are relaxed on the grid,
        one launch more, before they go back to spectra.  slots=True: the slot analysis (spdy_slot_ens_letkf_dev), as
        analyse_grid's; the launch count is that of the plain call."""
        self._analyse(self.lib.spdy_ens_letkf_dev, self.lib.spdy_mask_ens_letkf_dev, self.lib.spdy_slot_ens_letkf_dev,
                      (vor, div, t, q, ps), use_mask(use, self.nmem, self._device()), slots)
