"""The nature run of a twin experiment on the device (spdy_nature_* in include/spdy.h, "nature run").

A Nature belongs to a plan.  It holds the gridded truth (set_state: one state's time level 1), writes the observation values of a
Letkf's current network from it with reproducible counter-based noise (observe), and scores an ensemble against it (verify): the
area-weighted rmse and bias of the ensemble mean and the spread, per variable and level, into a slot of a small device table.
One cycle of a twin experiment is then a sequence of enqueues that one captured graph can hold:

    nature state's step; ens.step(...) x n; nat.set_state(...); nat.observe(letkf); ens.verify(letkf, nat, 0);
    ens.analyse(letkf); ens.verify(letkf, nat, 1); ens.startup(delt)

and the host reads scores() -- 3 (4 kx + 1) doubles per slot -- when it wants to look."""
import ctypes

from ._lib import check
from .columns import DeviceField, PlanObject
from .letkf import use_mask

_FIELDS = {"truth": lambda n: (4 * n.sp.kx + 1,) + n.sp.grid_shape, "scores": lambda n: (n.capacity, 3, 4 * n.sp.kx + 1),
           "state": lambda n: (2,)}   # device field -> its shape for a Nature n, all float64
NATURE_FIELDS = tuple(_FIELDS)
SCORES = ("rmse", "bias", "spread")


class Nature(PlanObject):
    """seed: of the observation noise; capacity: slots of the score table (>= 1).  The plan needs sigma levels and max_batch >=
    2 kx + 1."""
    PREFIX = "spdy_nature"

    def __init__(self, sp, seed=0, capacity=2):
        self.sp, self.lib = sp, sp.lib
        if sp.device >= 0:
            sp._sync_stream()
        h = ctypes.c_void_p()
        check(self.lib.spdy_nature_create(sp.h, int(seed) & 0xFFFFFFFFFFFFFFFF, int(capacity), ctypes.byref(h)))
        self.h, self.capacity = h, int(capacity)

    def _sync(self):
        if self.sp.device >= 0:
            self.sp._sync_stream()

    def _spectra(self, what, arrays, lead):
        """the five arrays of a time level as pointers: contiguous complex128 device tensors, vor .. q lead + (kx, nx, mx), ps lead +
        (nx, mx)"""
        import torch
        sp = self.sp
        shapes = [lead + (sp.kx, sp.nx, sp.mx)] * 4 + [lead + (sp.nx, sp.mx)]
        for a, s in zip(arrays, shapes):
            if tuple(a.shape) != s or a.dtype != torch.complex128 or not a.is_contiguous():
                raise ValueError("%s: expected a contiguous complex128 tensor of shape %s, got %s" % (what, s, tuple(a.shape)))
        return [ctypes.c_void_p(a.data_ptr()) for a in arrays]

    def set_state(self, vor, div, t, q, ps):
        """The truth from one state's time level 1: vor, div, t, q [kx, nx, mx], ps [nx, mx] complex128 device tensors (of
        Ensemble.member(e): D["vor"][0], .., D["tr"][0], D["ps"][0]).  One inverse batch, the analysis' own with one member;
        capturable."""
        ptrs = self._spectra("set_state", (vor, div, t, q, ps), ())
        self._sync()
        check(self.lib.spdy_nature_set_state_dev(self.h, *ptrs))

    def observe(self, letkf, noise=1.0, slot=None):
        """The values of letkf's current network (the latest set_obs; its values are ignored) from the truth: H(truth) + noise *
        error * z, z the standard normal draw of (seed, draws, observation).  Advances draws on the stream, so every replay of a
        captured observe draws fresh noise; noise = 0 gives H(truth) to the bit.  Two launches; capturable.
        slot: None, or a time slot of letkf.set_slots (include/spdy.h, "observations in time slots"): only that slot's observations
        get their values, from the truth as it stands now, with the draw the whole network's call would give them; the other values
        keep their bits; draws advances all the same.  Two launches, one for an empty slot."""
        if getattr(letkf, "sp", None) is not self.sp:
            raise ValueError("observe: the Letkf must belong to the nature run's plan")
        self._sync()
        if slot is None:
            check(self.lib.spdy_nature_observe_dev(self.h, letkf.h, float(noise)))
        else:
            check(self.lib.spdy_slot_nature_observe_dev(self.h, letkf.h, int(slot), float(noise)))

    def _device(self):
        return "cuda:%d" % self.sp.device if self.sp.device >= 0 else "cpu"

    def verify(self, letkf, vor, div, t, q, ps, slot=0, use=None):
        """Scores time level 1 of an ensemble of letkf.nmem members (vor .. q [nmem, kx, nx, mx], ps [nmem, nx, mx]) against the
        truth into scores[slot]; uses letkf's grid workspace, which the next analysis overwrites anyway.  Three launches;
        capturable.  Ensemble.verify passes the ensemble's arrays.  use: None, or the member mask (include/spdy.h, "member mask"; a
        sequence or a contiguous int32 device tensor of nmem entries): mean error, bias and spread over the members in use only;
        one of them gives spread 0, none NaN."""
        if getattr(letkf, "sp", None) is not self.sp:
            raise ValueError("verify: the Letkf must belong to the nature run's plan")
        use = use_mask(use, letkf.nmem, self._device())
        ptrs = self._spectra("verify", (vor, div, t, q, ps), (letkf.nmem,))
        self._sync()
        if use is None:
            check(self.lib.spdy_nature_verify_dev(self.h, letkf.h, *ptrs, int(slot)))
        else:
            check(self.lib.spdy_mask_nature_verify_dev(self.h, letkf.h, *ptrs, ctypes.c_void_p(use.data_ptr()), int(slot)))

    def verify_grid(self, ug, vg, tg, qg, psg, slot=0, use=None):
        """Scores an ensemble that is on the grid already (ug .. qg [nmem, kx, il, ix], psg [nmem, il, ix] float64 device tensors,
        Letkf.analyse_grid's layout) into scores[slot].  Two launches; capturable.  use: as verify's."""
        import torch
        sp, E = self.sp, int(psg.shape[0])
        use = use_mask(use, E, self._device())
        x = (ug, vg, tg, qg, psg)
        for a, s in zip(x, [(E, sp.kx) + sp.grid_shape] * 4 + [(E,) + sp.grid_shape]):
            if tuple(a.shape) != s or a.dtype != torch.float64 or not a.is_contiguous():
                raise ValueError("verify_grid: expected a contiguous float64 tensor of shape %s, got %s" % (s, tuple(a.shape)))
        self._sync()
        ptrs = [ctypes.c_void_p(a.data_ptr()) for a in x]
        if use is None:
            check(self.lib.spdy_nature_verify_grid_dev(self.h, E, *ptrs, int(slot)))
        else:
            check(self.lib.spdy_mask_nature_verify_grid_dev(self.h, E, *ptrs, ctypes.c_void_p(use.data_ptr()), int(slot)))

    def field(self, name):
        """A DeviceField in the object's own memory (NATURE_FIELDS): truth [4 kx + 1, il, ix] (u, v, t, q by level, then ps),
        scores [capacity, 3, 4 kx + 1], state [2] (the words seed and draws, as the bits of two doubles)."""
        p = ctypes.c_void_p()
        check(self.lib.spdy_nature_field(self.h, name.encode(), ctypes.byref(p)))
        return DeviceField(self.sp, p.value, _FIELDS[name](self))

    def truth(self):
        """{"u", "v", "t", "q": [kx, il, ix], "ps": [il, ix]} as NumPy (synchronising)"""
        g, kx = self.field("truth").numpy(), self.sp.kx
        out = {v: g[n * kx:(n + 1) * kx] for n, v in enumerate(("u", "v", "t", "q"))}
        out["ps"] = g[4 * kx]
        return out

    def scores(self, slot=None):
        """{"rmse" | "bias" | "spread": {"u", "v", "t", "q": [kx], "ps": float}} of a slot as NumPy; slot=None: every slot, stacked
        in front ([capacity, kx] and [capacity]).  Synchronising: it waits for everything enqueued on the plan's stream."""
        if slot is not None and not 0 <= int(slot) < self.capacity:
            raise ValueError("scores: slot %d outside [0, %d)" % (slot, self.capacity))
        table, kx = self.field("scores").numpy(), self.sp.kx
        if slot is not None:
            table = table[int(slot)]
        out = {}
        for n, name in enumerate(SCORES):
            row = table[..., n, :]
            out[name] = {v: row[..., i * kx:(i + 1) * kx] for i, v in enumerate(("u", "v", "t", "q"))}
            out[name]["ps"] = float(row[4 * kx]) if slot is not None else row[..., 4 * kx]
        return out

    def draws(self):
        """The number of observe calls since create / reset (downloads the device counter: synchronises the plan's stream)."""
        self._sync()
        n = ctypes.c_longlong()
        check(self.lib.spdy_nature_draws(self.h, ctypes.byref(n)))
        return n.value

    def reset(self, seed):
        """A new seed and draws = 0: the next observe draws what a fresh object with that seed draws.  Stream-ordered; not during a
        capture."""
        self._sync()
        check(self.lib.spdy_nature_reset(self.h, int(seed) & 0xFFFFFFFFFFFFFFFF))
