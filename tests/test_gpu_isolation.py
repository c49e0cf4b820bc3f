"""GPU: a non-finite field or member never reaches its neighbours (include/spdy.h, "batches").

An output field depends on the inputs the reference reads for that field and on nothing else the batch holds.  The finite-data
tests cannot tell a kernel that keeps to this from one that mixes two fields through a zero table entry, a shared reduction or a
two-for-one FFT: x + 0 * y is x for every finite y.  Here y is NaN, infinite or 1e300 (tests/poison.py).

The one assertion, everywhere: the call runs twice on one plan at one size -- both runs take the same launch form -- once on
clean inputs, once with chosen fields or members poisoned, and
  1. every output the reference computes without reading a poisoned input has the clean run's BITS;
  2. every output the reference does compute from a poisoned input shows the poison (poison.reached);
  3. the inputs equal their copies afterwards and the sentinels around the outputs (guards.Guarded) are intact;
  4. the clean run is anchored once to the oracle at conftest.TOL on a sample of fields.

  part 1  test_transform_*, test_four_kernel_*, test_stage_*: the transform entry points in every launch form guards.route names
          on this device, the four-kernel path, the stage calls
  part 2  test_dead_entries_*: the entries the inverse transform never reads (l > trunc + 1, Im(m' = 0)) hold NaN / inf -- in
          every inverse form and in the plain segments of a mixed launch (test_gpu_parity.py has the host entry points)
  part 3  test_ensemble_step_*: the ensemble step where T30 tiles and T63 pairs straddle members
  part 4  test_column_physics_*, test_ensemble_physics_*: the column physics with a non-finite state beside healthy ones
  part 5  test_member_goes_nonfinite_in_a_coupled_run: a member turns NaN in the middle of a coupled ensemble run

Sizes come from guards.route itself: for every entry point the smallest odd batch from 3 up that route sends to each form.  The
forms that cannot be reached on a device are those route never returns for it (T63 "resident" with 256 CUs: a launch with more
pairs than half the CUs holds 36 MiB of grids or more, and streams).
"""
import numpy as np
import pytest

import diagnostics as dg
import ensemblestep as es
import levels
import moist
import physlevels as pl
import physstep
import poison
import support
import synth
from conftest import TOL
from dynstep import ROB, oracle_dynamics_step, wave_relerr
from guards import GRID_BYTES, STREAM_MIN, Guarded, mixed_units, pin_launch_options, route, route_units

pytestmark = pytest.mark.gpu

MAX_BATCH = 512
FORMS = {("t30", "s2g"): ("part", "resident", "stream"), ("t30", "g2s"): ("split", "resident", "stream"),
         ("t63", "s2g"): ("chunk", "chunk_wt", "resident", "stream"), ("t63", "g2s"): ("staged", "split", "resident", "stream")}
OPS = {"spec_to_grid": "s2g", "grid_to_spec": "g2s", "uvspec_to_grid": "s2g", "grad_to_grid": "s2g", "vdspec": "g2s",
       "inverse_segs": "s2g", "direct_batch": "g2s"}
DEFAULT_CUS = 256                     # an MI355X; used to name the cases where no device is visible (they do not run there)


def num_cu():
    try:
        import torch
        if torch.cuda.is_available():
            return torch.cuda.get_device_properties(0).multi_processor_count
    except Exception:
        pass
    return DEFAULT_CUS


def seg_sizes(n):
    """the four plain segments of the mixed inverse call at size n: unequal, odd"""
    return (n, n + 2, n + 4, n + 6)


def op_route(tag, op, n, n_cu):
    """The launch form of entry point `op` at size n (n fields, or n pairs; inverse_segs: n pairs, seg_sizes(n), n gradients;
    direct_batch: n pairs and n + 2 plain fields), from guards.route and the builders in csrc/spdy_api.hip."""
    d = OPS[op]
    if op in ("spec_to_grid", "grid_to_spec"):
        return route(tag, d, n, n_cu, max_batch=MAX_BATCH)
    if op in ("uvspec_to_grid", "grad_to_grid", "vdspec"):
        return route(tag, d, n, n_cu, pairs=True, max_batch=MAX_BATCH)
    if op == "inverse_segs":
        units, fields, _ = mixed_units(tag, d, n, seg_sizes(n), n)
        return route_units(tag, d, units, fields, n_cu)
    if tag == "t30" and (3 * n + 2) * GRID_BYTES[tag] >= STREAM_MIN:
        # direct_batch at T30 from the streaming size on: the pairs and the plain fields as a launch each (one_mixed_launch)
        a, b = route(tag, d, n, n_cu, pairs=True), route(tag, d, n + 2, n_cu)
        return a if a == b else a + "+" + b
    units, fields, staged = mixed_units(tag, d, n, (n + 2,))
    return route_units(tag, d, units, fields, n_cu, staged_units=staged, max_batch=MAX_BATCH)


def sizes(tag, op, n_cu):
    """{form: the smallest odd n >= 3 that reaches it} for every form of FORMS that route returns for `op` on n_cu CUs"""
    out = {}
    for n in range(3, MAX_BATCH - 6, 2):
        out.setdefault(op_route(tag, op, n, n_cu), n)
    return {f: out[f] for f in FORMS[(tag, OPS[op])] if f in out}


def transform_cases():
    n_cu, cases = num_cu(), []
    for tag in ("t30", "t63"):
        for op in OPS:
            for form, n in sizes(tag, op, n_cu).items():
                cases.append((tag, op, form, n))
    return cases


CASES = transform_cases()
# the forms of FORMS that no size reaches, by CU count: T63 "resident" with 256 CUs -- a launch with more pairs than half the CUs
# holds more than 256 fields, 36 MiB of grids, and streams
UNREACHED = {256: {("t63", "s2g", "resident"), ("t63", "g2s", "resident")}}
POSITIONS = ("first", "second", "last", "later")


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def many(make, n, uniq=32):
    """n distinct fields from `uniq` seeded ones: field b is field b % uniq times 1 + (b // uniq) / 16 (on the device)"""
    import torch
    base = to_dev(make(min(n, uniq)))
    reps = -(-n // uniq)
    scale = 1.0 + torch.arange(reps, dtype=torch.float64, device="cuda").repeat_interleave(base.shape[0])[:n] / 16.0
    return (base.repeat((reps,) + (1,) * (base.dim() - 1))[:n] * scale.view((n,) + (1,) * (base.dim() - 1))).contiguous()


def _pinned_plan(tag):
    import speedy_f90_amd as s
    sp = s.Spectral(tag, kx=8, max_batch=MAX_BATCH, device=0)
    pin_launch_options(sp)
    return sp


@pytest.fixture(scope="module")
def plans():
    with support.plan_cache(_pinned_plan) as cached:
        def get(tag, fused=-1):
            sp = cached(tag)
            sp.set_fused(fused)
            return sp
        yield get


@pytest.fixture(scope="module", autouse=True)
def close_shared_plans():
    """the plans the shared clean runs keep (one per part at a time) go when the module is done"""
    yield
    for cache in (_ens_clean, _phys_clean, _ens_phys_clean, _coupled):
        if "sp" in cache:
            cache["sp"].close()
        cache.clear()
    _clean.clear()
    _stage_clean.clear()


# ------------------------------------------------------------------------------------------------ part 1: the entry points
class Call:
    """One entry point at one size: the clean inputs, how to run it into guarded outputs, which outputs an input field reaches,
    where the four poisoned positions are, and the oracle's value of one output field."""

    def __init__(self, sp, op, n, seed):
        import torch
        self.sp, self.op, self.n = sp, op, n
        spec = lambda k, first: many(lambda m: synth.spectra(m, sp.trunc, first=seed + first, full_rows=True), k)
        grid = lambda k, first: many(lambda m: synth.grids(m, sp.ix, sp.il, first=seed + first), k)
        self.complex_out = OPS[op] == "g2s"
        last = n - 1
        if op == "spec_to_grid":
            self.inputs = {"spec": spec(n, 0)}
            self.kcos = [2 if b % 3 == 1 else 1 for b in range(n)]
            self.d_kcos = torch.tensor(self.kcos, dtype=torch.int32, device="cuda")
            self.counts = [n]
            self.where = {"first": ("spec", 0), "second": ("spec", 1), "last": ("spec", last)}
        elif op == "grid_to_spec":
            self.inputs = {"grid": grid(n, 0)}
            self.counts = [n]
            self.where = {"first": ("grid", 0), "second": ("grid", 1), "last": ("grid", last)}
        elif op == "uvspec_to_grid":
            self.inputs = {"vor": spec(n, 0), "div": spec(n, 40)}
            self.counts = [n, n]
            self.where = {"first": ("vor", 0), "second": ("vor", 1), "last": ("div", last), "later": ("div", 0)}
        elif op == "grad_to_grid":
            self.inputs = {"psi": spec(n, 0)}
            self.counts = [n, n]
            self.where = {"first": ("psi", 0), "second": ("psi", 1), "last": ("psi", last)}
        elif op == "vdspec":
            self.inputs = {"ug": grid(n, 0), "vg": grid(n, 40)}
            self.counts = [n, n]
            self.where = {"first": ("ug", 0), "second": ("ug", 1), "last": ("vg", last), "later": ("vg", 0)}
        elif op == "inverse_segs":
            self.segs = seg_sizes(n)
            self.inputs = {"vor": spec(n, 0), "div": spec(n, 40), "psi": spec(n, 80)}
            for i, m in enumerate(self.segs):
                self.inputs["seg%d" % i] = spec(m, 120 + 40 * i)
            self.counts = [n, n, sum(self.segs), n, n]
            # second: inside the first plain segment; later: the first field of the second segment -- at T30, where tiles are
            # cut from the concatenated segments and the first is odd, the second field of a tile that straddles two arrays
            self.where = {"first": ("vor", 0), "second": ("seg0", 1), "later": ("seg1", 0), "last": ("psi", last)}
        else:
            self.inputs = {"ug": grid(n, 0), "vg": grid(n, 40), "plain": grid(n + 2, 80)}
            self.counts = [n, n, n + 2]
            self.where = {"first": ("ug", 0), "second": ("vg", 1), "later": ("plain", 0), "last": ("plain", n + 1)}

    def outputs(self):
        import torch
        shape = (self.sp.nx, self.sp.mx) if self.complex_out else (self.sp.il, self.sp.ix)
        return Guarded(torch, shape, self.counts, complex_=self.complex_out)

    def run(self, x, out):
        sp, op, o = self.sp, self.op, out.outs
        if op == "spec_to_grid":
            sp.spec_to_grid_dev(x["spec"], o[0], d_kcos=self.d_kcos)
        elif op == "grid_to_spec":
            sp.grid_to_spec_dev(x["grid"], o[0])
        elif op == "uvspec_to_grid":
            sp.uvspec_to_grid_dev(x["vor"], x["div"], o[0], o[1], 2)
        elif op == "grad_to_grid":
            sp.grad_to_grid_dev(x["psi"], o[0], o[1], 2)
        elif op == "vdspec":
            sp.vdspec_dev(x["ug"], x["vg"], o[0], o[1], 2)
        elif op == "inverse_segs":
            sp.inverse_batch_segs_dev(x["vor"], x["div"], o[0], o[1], [x["seg%d" % i] for i in range(4)], o[2], x["psi"], o[3], o[4],
                                      kcos_pairs=2, kcos=1, kcos_grad=2)
        else:
            sp.direct_batch_dev(x["ug"], x["vg"], o[0], o[1], x["plain"], o[2], 2)
        sp.synchronize()

    def reaches(self, name, k):
        """[(output, field)] the reference computes from input field (name, k)"""
        op = self.op
        if op in ("spec_to_grid", "grid_to_spec"):
            return [(0, k)]
        if op in ("uvspec_to_grid", "grad_to_grid", "vdspec"):
            return [(0, k), (1, k)]
        if name.startswith("seg"):
            return [(2, sum(self.segs[:int(name[3:])]) + k)]
        if name == "psi":
            return [(3, k), (4, k)]
        return [(2, k)] if name == "plain" else [(0, k), (1, k)]

    def reference(self, o, i, k):
        """the oracle's output field (i, k) from the device's own clean inputs"""
        op = self.op
        h = lambda name, j: self.inputs[name][j].cpu().numpy()
        if op == "spec_to_grid":
            return o.spec_to_grid(h("spec", k), self.kcos[k])
        if op == "grid_to_spec" or (op == "direct_batch" and i == 2):
            return o.grid_to_spec(h("grid" if op == "grid_to_spec" else "plain", k))
        if op in ("vdspec", "direct_batch"):
            return o.vdspec(h("ug", k), h("vg", k), 2)[i]
        if op == "grad_to_grid" or (op == "inverse_segs" and i >= 3):
            return o.spec_to_grid(o.grad(h("psi", k))[i - 3 if op == "inverse_segs" else i], 2)
        if op == "uvspec_to_grid" or i < 2:
            return o.spec_to_grid(o.uvspec(h("vor", k), h("div", k))[i], 2)
        s = 0
        while k >= self.segs[s]:
            k -= self.segs[s]
            s += 1
        return o.spec_to_grid(h("seg%d" % s, k), 1)


_clean = {}


def clean_run(key, make, o):
    """The clean run of `key`, made once and shared by its poisoned cases: (call, copies of its outputs).  The run is checked
    here: sentinels, inputs, and the oracle on the fields the poisoned positions reach and on their tile or pair partners."""
    import torch
    if _clean.get("key") != key:
        _clean.clear()
        call = make()
        copies = {k: v.clone() for k, v in call.inputs.items()}
        out = call.outputs()
        torch.cuda.synchronize()
        call.run(call.inputs, out)
        assert out.intact(), "%s clean: sentinel fields overwritten at (band, field) %s" % (key, out.hits()[:8])
        for k, v in call.inputs.items():
            assert torch.equal(v, copies[k]), "%s clean: input %s changed" % (key, k)
        sample = set()
        for name, k in call.where.values():
            for i, f in call.reaches(name, k):
                sample |= {(i, f), (i, f ^ 1 if (f ^ 1) < call.counts[i] else f)}
        worst = 0.0
        for i, f in sorted(sample):
            e = synth.relerr(out.outs[i][f].cpu().numpy(), call.reference(o, i, f))
            assert e <= TOL, "%s clean: output %d field %d differs from the oracle by %r" % (key, i, f, e)
            worst = max(worst, e)
        print("\n[%s] clean run: %d fields against the oracle, worst %.2e" % (" ".join(str(k) for k in key), len(sample), worst))
        _clean.update(key=key, call=call, outs=[x.clone() for x in out.outs])
    return _clean["call"], _clean["outs"]


def check_poisoned(label, call, clean, kind, position):
    """assertions 1-3 of the poisoned run"""
    import torch
    name, k = call.where[position]
    x = {n: v.clone() for n, v in call.inputs.items()}
    poison.poison(x[name][k], kind)
    copies = {n: v.clone() for n, v in x.items()}
    out = call.outputs()
    torch.cuda.synchronize()
    call.run(x, out)
    assert out.intact(), "%s: sentinel fields overwritten at (band, field) %s" % (label, out.hits()[:8])
    for n, v in x.items():
        assert support.same_bits(v, copies[n]), "%s: input %s changed" % (label, n)
    hit, shown = call.reaches(name, k), []
    for i, (got, want) in enumerate(zip(out.outs, clean)):
        mine = [f for j, f in hit if j == i]
        keep = torch.ones(got.shape[0], dtype=torch.bool, device=got.device)
        if mine:
            keep[mine] = False
        a, b = (torch.view_as_real(t) if t.is_complex() else t for t in (got, want))
        diff = (a.view(torch.int64) != b.view(torch.int64)).flatten(1).any(1) & keep
        assert not bool(diff.any()), "%s: %s[%d] poisoned, output %d fields %s changed" % (label, name, k, i, diff.nonzero().flatten().tolist()[:8])
        shown += [(i, f) for f in mine if poison.reached(got[f], kind)]
    # every output the input reaches shows the poison.  The finite kind is a zonally constant field: where the reference's own
    # result for such an input is an exact zero times it (the divergence of a zonally constant u, the vorticity of such a v), the
    # output holds no trace of it, so there one of the pair's two outputs has to show it.
    missing = [x for x in hit if x not in shown]
    assert not missing if kind != "1e300" else shown, "%s: %s[%d] poisoned, outputs (output, field) %s do not show it" % (label, name, k, missing)


def _transform_params():
    out = []
    for tag, op, form, n in CASES:
        for kind in (("nan",) if form == "stream" else poison.KINDS):
            for pos in POSITIONS:
                if pos == "later" and op in ("spec_to_grid", "grid_to_spec", "grad_to_grid"):
                    continue                                     # one input array, one segment
                out.append(pytest.param(tag, op, form, n, kind, pos, id="%s-%s-%s-n%d-%s-%s" % (tag, op, form, n, kind, pos)))
    return out


@pytest.mark.parametrize("tag,op,form,n,kind,position", _transform_params())
def test_transform_entry_point(tag, op, form, n, kind, position, plans, oracle_factory):
    """A device-pointer entry point in one launch form (asserted from guards.route and the device's CU count), one field of one
    input poisoned: field 0, the second field of a T30 tile or T63 pair, the last field (alone in its tile or pair) or the first
    field of a later segment.  For the pair operators a poisoned vor[k] / div[k] / ug[k] / vg[k] reaches both outputs k."""
    import torch
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    got = op_route(tag, op, n, n_cu)
    print("\n[%s %s n=%d] %d CUs: route %s" % (tag, op, n, n_cu, got))
    assert got == form, (tag, op, n, n_cu, got, form)
    sp = plans(tag)
    key = (tag, op, form, n)
    call, clean = clean_run(key, lambda: Call(sp, op, n, 6100), oracle_factory(tag))
    check_poisoned("%s %s %s n=%d %s %s" % (tag, op, form, n, kind, position), call, clean, kind, position)


def test_every_form_is_reached():
    """On this device every entry point reaches every form guards.route names for its direction, but for the listed exceptions: a
    form that drops out of the parametrisation on a device with another CU count fails here instead of vanishing."""
    import torch
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    assert n_cu == num_cu()
    for tag in ("t30", "t63"):
        for op, d in OPS.items():
            missing = {(tag, d, f) for f in FORMS[(tag, d)] if f not in sizes(tag, op, n_cu)}
            assert missing == {x for x in UNREACHED.get(n_cu, set()) if x[:2] == (tag, d)}, (op, n_cu, missing)
            assert {c[2]: c[3] for c in CASES if c[:2] == (tag, op)} == sizes(tag, op, n_cu), (tag, op)


FOUR_N = 9      # the four-kernel path: odd, several workgroups of every stage kernel


@pytest.mark.parametrize("position", ("first", "second", "last"))
@pytest.mark.parametrize("kind", poison.KINDS)
@pytest.mark.parametrize("op", ("spec_to_grid", "grid_to_spec"))
@pytest.mark.parametrize("tag", ("t30", "t63"))
def test_four_kernel_path(tag, op, kind, position, plans, oracle_factory):
    """The two plain transforms on the four-kernel path (set_fused(0)): Legendre and Fourier stages through the plan's workspace."""
    sp = plans(tag, fused=0)
    try:
        call, clean = clean_run((tag, op, "four-kernel", FOUR_N), lambda: Call(sp, op, FOUR_N, 6300), oracle_factory(tag))
        check_poisoned("%s %s four-kernel %s %s" % (tag, op, kind, position), call, clean, kind, position)
    finally:
        sp.set_fused(-1)


STAGES = {"legendre_inv": ("spec", "legendre_inv"), "fourier_inv": ("four", "fourier_inv"), "fourier_dir": ("grid", "fourier_dir"),
          "legendre_dir": ("four", "legendre_dir")}
_stage_clean = {}


def stage_input(sp, o, stage, nb, seed):
    """nb ordinary inputs of a stage call: spectra, grids, or the Fourier rows the stage in front of it makes of them"""
    kind = STAGES[stage][0]
    if kind == "spec":
        return synth.spectra(nb, sp.trunc, first=seed, full_rows=True)
    if kind == "grid":
        return synth.grids(nb, sp.ix, sp.il, first=seed)
    if stage == "fourier_inv":
        return np.stack([o.legendre_inv(s) for s in synth.spectra(nb, sp.trunc, first=seed, full_rows=True)])
    return np.stack([o.fourier_dir(g) for g in synth.grids(nb, sp.ix, sp.il, first=seed)])


def stage_call(sp, stage, x):
    return sp.fourier_inv(x, 2) if stage == "fourier_inv" else getattr(sp, stage)(x)


@pytest.mark.parametrize("position", (0, 1, 2))
@pytest.mark.parametrize("kind", poison.KINDS)
@pytest.mark.parametrize("stage", tuple(STAGES))
@pytest.mark.parametrize("tag", ("t30", "t63"))
def test_stage_call(tag, stage, kind, position, plans, oracle_factory):
    """legendre_inv, fourier_inv, fourier_dir, legendre_dir on their own at nb = 3 (host arrays: the outputs are the wrapper's own
    arrays, so there are no sentinels to check)."""
    sp, o = plans(tag, fused=0), oracle_factory(tag)
    key = (tag, stage)
    if key not in _stage_clean:
        x = stage_input(sp, o, stage, 3, 6400)
        y = stage_call(sp, stage, x)
        ref = np.stack([o.fourier_inv(f, 2) if stage == "fourier_inv" else getattr(o, stage)(f) for f in x])
        for b in range(3):
            assert synth.relerr(y[b], ref[b]) <= TOL, (tag, stage, b)
        _stage_clean[key] = (x, y)
    x, clean = _stage_clean[key]
    bad = x.copy()
    poison.poison(bad[position], kind)
    copy = bad.copy()
    got = stage_call(sp, stage, bad)
    sp.set_fused(-1)
    assert support.same_bits(bad, copy), "input changed"
    for b in range(3):
        if b == position:
            assert poison.reached(got[b], kind), (tag, stage, kind, "field %d does not show the poison" % b)
        else:
            assert support.same_bits(got[b], clean[b]), (tag, stage, kind, "field %d poisoned, field %d changed" % (position, b))


# ------------------------------------------------------------------------------- part 2: the entries the reference never reads
DEAD = ("dead-nan", "dead-inf", "im0-nan")


def fill_dead(spec, sp, what):
    """in place on a stack of spectra [nb, nx, mx] (device): every entry with l > trunc + 1 set to nan + nan j / inf - inf j, or
    Im(m' = 0) of every row set to NaN"""
    import torch
    nan, inf = float("nan"), float("inf")
    if what == "im0-nan":
        torch.view_as_real(spec)[:, :, 0, 1] = nan
    else:
        mask = to_dev(poison.dead_mask(sp.nx, sp.mx, sp.trunc))
        spec[:, mask] = complex(nan, nan) if what == "dead-nan" else complex(inf, -inf)
    return spec


INVERSE_CASES = [c for c in CASES if c[1] in ("spec_to_grid", "inverse_segs")]


@pytest.mark.parametrize("what", DEAD)
@pytest.mark.parametrize("tag,op,form,n", INVERSE_CASES, ids=["%s-%s-%s-n%d" % c for c in INVERSE_CASES])
def test_dead_entries_every_inverse_form(tag, op, form, n, what, plans, oracle_factory):
    """spec_to_grid_dev in every inverse form, and the plain segments of inverse_batch_segs_dev: with non-finite values in every
    entry the reference never reads, EVERY output field has the clean run's bits.  (The operator inputs of the mixed call stay
    clean: uvspec and grad read entry n + 1 of the dead part whatever it holds, and so do the kernels.)"""
    import torch
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    assert op_route(tag, op, n, n_cu) == form, (tag, op, n, n_cu, op_route(tag, op, n, n_cu), form)
    sp = plans(tag)
    call, clean = clean_run((tag, op, form, n), lambda: Call(sp, op, n, 6100), oracle_factory(tag))
    x = {k: v.clone() for k, v in call.inputs.items()}
    for k in x:
        if k == "spec" or k.startswith("seg"):
            fill_dead(x[k], sp, what)
    copies = {k: v.clone() for k, v in x.items()}
    out = call.outputs()
    torch.cuda.synchronize()
    call.run(x, out)
    assert out.intact(), out.hits()[:8]
    for k, v in x.items():
        assert support.same_bits(v, copies[k]), "input %s changed" % k
    for i, (got, want) in enumerate(zip(out.outs, clean)):
        diff = (got.view(torch.int64) != want.view(torch.int64)).flatten(1).any(1)
        assert not bool(diff.any()), "%s %s %s n=%d %s: output %d fields %s changed" % (tag, op, form, n, what, i, diff.nonzero().flatten().tolist()[:8])


@pytest.mark.parametrize("what", ["nan", "inf"])
def test_guard_ignores_the_zonal_column(what):
    """The guard's sums skip zonal wavenumber 0 of vor and div, which the reference's loops never read (diagnostics.f90; DESIGN.md
    s16: "dropped by a select, not multiplied by zero").  One Diagnostics of three members: with that column of member 1's vor and
    div NaN, or +inf / -inf, every member's row -- member 1's too -- has the clean check's bits and no member is flagged.  A NaN in a
    coefficient that is read flags member 1 alone and leaves the rows of members 0 and 2 as they were."""
    s = support.package()
    E = 3
    sp = support.plan("t30", max_batch=4)
    x = {n: np.stack([dg.state(sp, 5700 + 100 * e)[n] for e in range(E)]) for n in ("vor", "div", "t")}
    G = s.Diagnostics(sp, capacity=4, first_step=0, nmem=E)
    check = lambda y: G.check_dev(*[support.dev(y[n]) for n in ("vor", "div", "t")])
    check(x)
    clean = np.stack([G.read(0, 1, member=e)[0] for e in range(E)])
    assert np.isfinite(clean).all() and not np.array_equal(clean[0], clean[2])
    y = {n: a.copy() for n, a in x.items()}
    for n in ("vor", "div"):
        y[n][1, :, :, 0] = complex(float("nan"), float("nan")) if what == "nan" else complex(float("inf"), -float("inf"))
    check(y)
    got = np.stack([G.read(1, 1, member=e)[0] for e in range(E)])
    assert support.same_bits(got, clean), "a value in the zonal column reached a sum"
    assert G.stopped() == [-1] * E
    y["div"][1, 2, 3, 2] = complex(float("nan"), 0.0)
    check(y)
    got = np.stack([G.read(2, 1, member=e)[0] for e in range(E)])
    assert support.same_bits(got[[0, 2]], clean[[0, 2]]) and np.isnan(got[1, 1, 2]) and G.stopped() == [-1, 2, -1]
    G.close()
    sp.close()


# --------------------------------------------------------------------------------------------------- part 3: the ensemble step
# (name, plan, oracle, E, time step, poisoned members)
def _t63_9(nmem):
    return levels.plan("t63", 9, nmem * (4 * 9 + 4))


ENSEMBLES = {"t30k5-E3": (lambda E: support.plan("t30k5", E * (4 * 5 + 4)), lambda f: f("t30k5"), 3, 2400.0),
             "t63k16-E3": (lambda E: support.plan("t63k16", E * (4 * 16 + 4)), lambda f: f("t63k16"), 3, 1200.0),
             "t63k9-E2": (_t63_9, lambda f: levels.oracle("t63", 9), 2, 1200.0)}
ENS_CASES = [("t30k5-E3", 1), ("t63k16-E3", 1), ("t63k9-E2", 1), ("t63k9-E2", 0)]
ENS_POISON = ("all-nan", "ps-inf", "t11-inf")
_ens_clean = {}


def ens_poison(ens, e, how):
    nan, inf = float("nan"), float("inf")
    if how == "all-nan":
        for n in es.PROG:
            getattr(ens, n)[:, e] = complex(nan, nan)
    elif how == "ps-inf":
        ens.ps[:, e] = complex(inf, 0.0)                          # both time levels
    else:
        ens.t[:, e, ens.kx - 1, 1, 1] = complex(inf, 0.0)         # coefficient (n, m') = (1, 1) of the lowest level


def ens_clean(name, oracle_factory):
    """The clean ensemble run of configuration `name` (two leapfrog steps), kept with its plan for the poisoned cases; member 0's
    first step is anchored to the oracle's call-by-call step as test_gpu_ensemble.py::test_member_zero_against_oracle does."""
    if _ens_clean.get("name") != name:
        if "sp" in _ens_clean:
            _ens_clean["sp"].close()
        _ens_clean.clear()
        make_plan, make_oracle, E, dt = ENSEMBLES[name]
        sp, o = make_plan(E), make_oracle(oracle_factory)
        sts = es.member_states(sp, E)
        snaps = es.run_ensemble(sp, es.build(sp, sts), es.LEAPFROG, dt)
        o.tail_init(dt)
        new, out = oracle_dynamics_step(o, sts[0], 2, dt, ROB)
        m = es.member_of(snaps[0], 0)
        for k in ("U", "PL"):
            assert synth.relerr(m[k].cpu().numpy(), out[k]) <= TOL, (name, k)
        for k in ("vor", "t", "ps"):
            g = m[k].cpu().numpy()
            assert synth.relerr(g, new[k]) <= TOL and wave_relerr(g, new[k]) <= TOL, (name, k)
        _ens_clean.update(name=name, sp=sp, sts=sts, snaps=snaps)
    return _ens_clean["sp"], _ens_clean["sts"], _ens_clean["snaps"]


@pytest.mark.parametrize("how", ENS_POISON)
@pytest.mark.parametrize("name,member", ENS_CASES, ids=["%s-member%d" % c for c in ENS_CASES])
def test_ensemble_step_member_isolated(name, member, how, oracle_factory):
    """Two leapfrog steps of an ensemble whose launches put two members into one T30 tile or T63 pair: T30 kx = 5, E = 3 (tiles of
    two fields over member stacks of 5 levels); T63 L16, E = 3 (the ps segment pairs member 0 with member 1); T63 at 9 levels, E = 2
    (every level segment pairs member 0's last level with member 1's first).  One member is poisoned -- all prognostics NaN; ps of
    both time levels +inf; coefficient (1, 1) of t at the lowest level +inf -- and every other member has the bits of the clean run
    of the same ensemble after each step, the poisoned member's vor is non-finite at the end, the shared fields are untouched."""
    E, dt = ENSEMBLES[name][2:]
    sp, sts, clean = ens_clean(name, oracle_factory)
    ens = es.build(sp, sts)
    ens_poison(ens, member, how)
    shared = {n: getattr(ens, n).clone() for n in ("phis", "tcorh", "qcorh")}
    snaps = es.run_ensemble(sp, ens, es.LEAPFROG, dt)
    for e in range(E):
        if e == member:
            continue
        for n, (got, want) in enumerate(zip(snaps, clean)):
            a, b = es.member_of(got, e), es.member_of(want, e)
            bad = [k for k in es.COMPARED if not support.same_bits(a[k], b[k])]
            assert bad == [], "%s, member %d %s: member %d step %d differs in %s" % (name, member, how, e, n + 1, bad)
    assert poison.nonfinite(snaps[-1]["vor"][:, member]), "%s, member %d %s: its vor is finite at the end" % (name, member, how)
    for n, v in shared.items():
        assert support.same_bits(getattr(ens, n), v), n


# --------------------------------------------------------------------- part 4: the column physics beside a non-finite state
# No memory index and no loop bound of the column kernels is made from a field value (DESIGN.md s5 lists each data-derived
# integer with the line that bounds it), so a non-finite state can be run beside healthy ones.
PHYS_LEVELS = (8, 12)              # T30 L8; 12 levels: the <16> kernels with unused levels (tests/physlevels.py)
PHYS_POISON = ("all-nan", "t-low-inf")
GRIDDED = ("ug", "vg", "tg", "qg", "phig", "pslg")
_phys_clean = {}


def _phys_plan(kx, max_batch=64):
    return (support.plan("t30", max_batch), moist.HSG[8]) if kx == 8 else (pl.plan(kx, max_batch), pl.hsg(kx))


def poison_state(d, b, how):
    """state b of the gridded inputs d (name -> [nb, ...] device tensors) in place: every gridded input NaN -- the six fields of the
    state, its boundary fields and its tendencies at entry -- or only its temperature +inf in the lowest level of every column"""
    if how == "all-nan":
        for v in d.values():
            v[b] = float("nan")
    else:
        d["tg"][b, -1] = float("inf")


def guarded_like(tensors, grid_shape):
    """tensors (float64 or int32, any shape) re-made as views into one Guarded allocation with a sentinel field in every gap; each
    takes whole fields, an int32 tensor the leading part of its last one"""
    import torch
    per = grid_shape[0] * grid_shape[1] * 8
    g = Guarded(torch, grid_shape, [max(1, -(-t.numel() * t.element_size() // per)) for t in tensors])
    views = []
    for t, o in zip(tensors, g.outs):
        flat = o.view(torch.int32).reshape(-1) if t.dtype == torch.int32 else o.reshape(-1)
        views.append(flat[:t.numel()].view(t.shape))
    return g, views


def run_chain(sp, nb, calls, sppt=None):
    """spdy_column_physics_dev (sppt = (pattern, mu): spdy_column_physics_sppt_dev) for each (inputs, shortwave) of `calls` on ONE
    radiation state, with the state, the tendencies and every optional output inside guard bands.  Returns (name -> tensor, the
    Guarded allocation)."""
    import torch
    S0 = torch.empty((nb * sp.radiation_state_size(),), dtype=torch.float64, device="cuda")
    outs = [sp.column_outputs(nb) for _ in calls]
    flat = [physstep.flat_outs(o) for o in outs]
    names = [("state", S0)] + [("%s%d" % (n, i + 1), d[n]) for i, (d, _) in enumerate(calls) for n in physstep.TEND]
    names += [("out%d.%s" % (i + 1, n), t) for i in range(len(calls)) for n, t in flat[i].items()]
    g, views = guarded_like([t for _, t in names], sp.grid_shape)
    V = dict(zip([n for n, _ in names], views))
    for i, (d, _) in enumerate(calls):
        for n in physstep.TEND:
            V["%s%d" % (n, i + 1)].copy_(d[n])
    for i, (d, sw) in enumerate(calls):
        out = {b: ({n: V["out%d.%s.%s" % (i + 1, b, n)] for n in v} if isinstance(v, dict) else V["out%d.%s" % (i + 1, b)])
               for b, v in outs[i].items()}
        if not sw:                         # ssrd stays where the shortwave call put it (include/spdy.h)
            out["rad"]["ssrd"] = V["out1.rad.ssrd"]
        args = (sw, d["ug"], d["vg"], d["tg"], d["qg"], d["phig"], d["pslg"], d, d["albsfc"], V["state"],
                *[V["%s%d" % (n, i + 1)] for n in physstep.TEND], out)
        if sppt is None:
            sp.column_physics_dev(*args)
        else:
            sp.column_physics_sppt_dev(sppt[0], sppt[1], *args)
    torch.cuda.synchronize()
    return V, g


def state_slices(V, nb, b):
    """name -> state b's part of everything run_chain wrote"""
    size = V["state"].numel() // nb
    return {n: (v[b * size:(b + 1) * size] if n == "state" else v[b]) for n, v in V.items()}


def phys_clean(kx, form, sppt):
    """the clean run of (kx, launch form, with SPPT), shared by its poisoned cases; its first call's tendencies are anchored to the
    chain of restatements (tests/surface.py, pinned to the reference by tests/golden) on every column -- with SPPT, to
    tests/sppt.py's formula applied to them with the run's own pattern and taper"""
    import radiation
    import sppt as spptref
    import surface
    key = (kx, form, sppt)
    if _phys_clean.get("key") != key:
        if "sp" in _phys_clean:
            _phys_clean["sp"].close()
        _phys_clean.clear()
        nb, keep = 3, {}
        sp, _, il, ix, d1, d2 = physstep.gridded("t30k%d" % kx, nb, 9700 + kx, plan=_phys_plan(kx), keep=keep)
        sp.column_physics_workspace()
        sp.set_option("physics_fused", 1 if form == "one-launch" else 0)
        pattern = None
        if sppt:
            sp.column_physics_sppt_workspace()
            P = np.clip(1.5 * (2.0 * synth.splitmix64(9760 + kx, nb * kx * il * ix) - 1.0), -1.0, 1.0).reshape(nb, kx, il, ix)
            pattern = (support.dev(P), spptref.mu(kx))
        calls = [(d1, True)] if sppt else [(d1, True), (d2, False)]
        V, g = run_chain(sp, nb, calls, pattern)
        assert g.intact(), g.hits()[:8]
        r, _ = surface.chain(keep["tab"], keep["c1"], keep["zon"], keep["sqcoa"])
        assert float(r["margin"].min()) >= surface.MIN_MARGIN
        for n in physstep.TEND:
            want = radiation.grids(r["pbl"][n], nb, il, ix)
            if sppt:                       # physics.f90:212-221 on the restatements' tendencies and the tendencies at entry
                want = np.moveaxis(spptref.apply(want.swapaxes(0, 1), np.moveaxis(d1[n].cpu().numpy(), 1, 0), np.moveaxis(P, 1, 0),
                                                 pattern[1]), 0, 1)
            e = synth.relerr(V[n + "1"].cpu().numpy(), want)
            assert e <= TOL, (kx, form, sppt, n, e)
        _phys_clean.update(key=key, sp=sp, nb=nb, calls=calls, pattern=pattern, V={n: v.clone() for n, v in V.items()})
    return _phys_clean


@pytest.mark.parametrize("how", PHYS_POISON)
@pytest.mark.parametrize("form,sppt", [("five-calls", False), ("one-launch", False), ("five-calls", True), ("one-launch", True)],
                         ids=["five-calls", "one-launch", "sppt-five-calls", "sppt-one-launch"])
@pytest.mark.parametrize("kx", PHYS_LEVELS)
def test_column_physics_state_isolated(kx, form, sppt, how):
    """spdy_column_physics_dev through the five calls and through the one launch, a shortwave call and then a call on the held
    radiation state, and spdy_column_physics_sppt_dev: three states, state 1 poisoned in both calls.  States 0 and 2 have the clean
    run's bits in the tendencies, every optional output (the integers iptop, icnv, icltop among them) and their slices of the
    radiation state; state 1's temperature tendency is non-finite; inputs and guard bands are unchanged."""
    c = phys_clean(kx, form, sppt)
    sp, nb = c["sp"], c["nb"]
    calls = [({n: v.clone() for n, v in d.items()}, sw) for d, sw in c["calls"]]
    for d, _ in calls:
        poison_state(d, 1, how)
    copies = [{n: v.clone() for n, v in d.items()} for d, _ in calls]
    V, g = run_chain(sp, nb, calls, c["pattern"])
    assert g.intact(), g.hits()[:8]
    for (d, _), cp in zip(calls, copies):
        for n, v in d.items():
            assert support.same_bits(v, cp[n]), "input %s changed" % n
    for b in (0, 2):
        got, want = state_slices(V, nb, b), state_slices(c["V"], nb, b)
        bad = [n for n in want if not support.same_bits(got[n], want[n])]
        assert bad == [], "%d levels %s sppt=%s %s: state %d differs in %s" % (kx, form, sppt, how, b, bad)
    mine = state_slices(V, nb, 1)
    for i in range(len(calls)):
        assert poison.nonfinite(mine["ttend%d" % (i + 1)]), "call %d: the poisoned state's ttend is finite" % (i + 1)
    assert {"out1.moist.iptop", "out1.moist.icnv", "out1.rad.icltop"} <= set(V)


_ens_phys_clean = {}


def ens_phys_run(sp, E, espec, ebnd, t0):
    """spdy_ens_physics_dev, a shortwave call and a call on the held state: every tendency, optional output and the radiation
    states, by name"""
    import torch
    S = torch.full((E * sp.radiation_state_size(),), float("nan"), dtype=torch.float64, device="cuda")
    res, ssrd = {"state": S}, None
    for i, sw in ((1, True), (2, False)):
        T, out = [t.clone() for t in t0], sp.column_outputs(E)
        if sw:
            ssrd = out["rad"]["ssrd"]
        else:
            out["rad"]["ssrd"] = ssrd
        sp.ens_physics_dev(E, sw, *espec, ebnd, ebnd["albsfc"], S, *T, out)
        res.update({"%s%d" % (n, i): t for n, t in zip(physstep.TEND, T)})
        res.update({"out%d.%s" % (i, n): t for n, t in physstep.flat_outs(out).items()})
    torch.cuda.synchronize()
    return res


def ens_phys_clean(kx, oracle_factory):
    """members, inputs and the clean run of spdy_ens_physics_dev at kx levels; member 0's tendencies of the shortwave call are
    anchored to the oracle's transforms and the chain of restatements (physstep.Case.physics)"""
    import torch
    if _ens_phys_clean.get("kx") != kx:
        if "sp" in _ens_phys_clean:
            _ens_phys_clean["sp"].close()
        _ens_phys_clean.clear()
        E = 3
        if kx == 8:
            sp, o, hsg, seeds = support.plan("t30", E * (4 * kx + 4)), oracle_factory("t30"), None, None
        else:
            sp, o, hsg, seeds = pl.levels_case(kx, E * (4 * kx + 4))
        sts, bnds = es.physics_members(sp, o, E, hsg, seeds)
        il, ix = sp.il, sp.ix
        dev = [physstep.device_boundary(b, il, ix) for b in bnds]
        ebnd = {n: torch.cat([b[n] for b in dev]) for n in dev[0]}
        spec = [[a for a in (st["vor"][0], st["div"][0], st["t"][0], st["tr"][0], o.geopotential(st["t"][0], st["phis"]), st["ps"][0])]
                for st in sts]
        espec = [support.dev(np.stack([spec[e][i] for e in range(E)])) for i in range(6)]
        host_t0 = [np.stack([synth.splitmix64(270 + 4 * e + i, kx * il * ix).reshape(kx, il, ix) * f for e in range(E)])
                   for i, f in enumerate((1e-4, 1e-4, 1e-4, 1e-7))]
        t0 = [support.dev(a) for a in host_t0]
        sp.ens_physics_workspace(E)
        clean = ens_phys_run(sp, E, espec, ebnd, t0)
        case = physstep.Case("t30", sp, o, st=sts[0], bnd=bnds[0], hsg=hsg)
        ref_t = [a[0].copy() for a in host_t0]
        case.physics(sts[0], True, {}, *ref_t)
        for n, w in zip(physstep.TEND, ref_t):
            e = synth.relerr(clean[n + "1"][0].cpu().numpy(), w)
            assert e <= TOL, (kx, n, e)
        _ens_phys_clean.update(kx=kx, sp=sp, E=E, espec=espec, ebnd=ebnd, t0=t0, clean=clean)
    return _ens_phys_clean


@pytest.mark.parametrize("how", PHYS_POISON)
@pytest.mark.parametrize("kx", PHYS_LEVELS)
def test_ensemble_physics_member_isolated(kx, how, oracle_factory):
    """spdy_ens_physics_dev from spectra, E = 3 with per-member boundary fields and radiation states: member 1's spectra (and, for
    "all-nan", its boundary fields and tendencies at entry) poisoned -- "t-low-inf": coefficient (0, 0) of its lowest-level
    temperature +inf, which the transform makes non-finite in every column of that level.  Members 0 and 2 have the clean run's bits
    everywhere; member 1's temperature tendency is non-finite."""
    c = ens_phys_clean(kx, oracle_factory)
    sp, E = c["sp"], c["E"]
    espec, ebnd, t0 = [x.clone() for x in c["espec"]], {n: v.clone() for n, v in c["ebnd"].items()}, [x.clone() for x in c["t0"]]
    nan, inf = float("nan"), float("inf")
    if how == "all-nan":
        for x in espec:
            x[1] = complex(nan, nan)
        for x in list(ebnd.values()) + t0:
            x[1] = nan
    else:
        espec[2][1, kx - 1, 0, 0] = complex(inf, 0.0)
    copies = [x.clone() for x in espec + list(ebnd.values()) + t0]
    got = ens_phys_run(sp, E, espec, ebnd, t0)
    for x, cp in zip(espec + list(ebnd.values()) + t0, copies):
        assert support.same_bits(x, cp), "an input changed"
    for b in (0, 2):
        a, w = state_slices(got, E, b), state_slices(c["clean"], E, b)
        bad = [n for n in w if not support.same_bits(a[n], w[n])]
        assert bad == [], "%d levels %s: member %d differs in %s" % (kx, how, b, bad)
    mine = state_slices(got, E, 1)
    assert poison.nonfinite(mine["ttend1"]) and poison.nonfinite(mine["ttend2"])


# ------------------------------------------------------------- part 5: a member goes non-finite in the middle of a coupled run
RUN_STEPS = 8
INJECT_AFTER = 2          # steps done when member 1's time-level-2 temperature is overwritten with NaN
RUN_WINDS = (0.0, 1.0e-5, 0.5e-5)     # longrun.rest_state's seeded vorticity amplitude per member: balanced states that differ
_coupled = {}


def coupled_setup(oracle_factory):
    """T30 L8, E = 3: the plan, the members' states (the reference's rest state with a different seeded wind each, over one
    orography), their boundary fields and the climatology -- states that run at the model's own time step"""
    import longrun
    import ensemblerun as er
    import surfmodel as sm
    if not _coupled:
        E = len(RUN_WINDS)
        sp, o = support.plan("t30", E * (4 * 8 + 4)), oracle_factory("t30")
        sts = [longrun.rest_state(o, wind=w) for w in RUN_WINDS]
        phis0 = o.spec_to_grid(sts[0]["phis"], 1)
        lat = longrun.latitudes(sp.table("sia_half"))
        bnds = [longrun.boundary(phis0, lat, 778 + e) for e in range(E)]
        clim = er.shaped(sm.climatology(phis0, lat), sp.grid_shape)
        sp.surface_set_orography(phis0)
        sp.initialize_implicit(longrun.DELT)
        sp.use_own_stream()
        _coupled.update(sp=sp, sts=sts, bnds=bnds, clim=clim, dt=longrun.DELT, runs={})
    return _coupled


def coupled_run(c, inject, graph):
    """RUN_STEPS steps of the coupled ensemble in the order of ensemblerun.run_ensemble -- {step, check_dev on time level 2,
    couple_dev(1)}, forcing_dev before a day's first step -- starting on the last step of a day, so that the second step is a
    day's first.  A single Diagnostics object follows member 1's slice.  inject: after INJECT_AFTER steps member 1's time-level-2
    t becomes NaN on the device.  Returns the snapshot after every step and the guards' final state."""
    import torch
    import ensemblerun as er
    import surfmodel as sm
    s = support.package()
    sp, sts, bnds, dt = c["sp"], c["sts"], c["bnds"], c["dt"]
    E = len(sts)
    ens = s.Ensemble(sp, E, member_qcorh=True)
    ens.set_shared(sts[0])
    for e, st in enumerate(sts):
        ens.set_member(e, st)
    M = s.SurfaceModel(sp, c["clim"], sm.DELT, nmem=E)
    G = s.Diagnostics(sp, capacity=RUN_STEPS, first_step=0, nmem=E)
    one_guard = s.Diagnostics(sp, capacity=RUN_STEPS, first_step=0)
    bnd, albsfc = M.boundary()
    out = sp.column_outputs(E, ("sfc", "rad"), names=er.FLUXES)
    F = dict(out["sfc"], **out["rad"])
    P = {"bnd": bnd, "albsfc": albsfc, "out": out,
         "rad": torch.full((E * sp.radiation_state_size(),), float("nan"), dtype=torch.float64, device="cuda")}
    er._start(M, bnds, E)
    M.forcing_dev(ens.qcorh)
    ens.physics_workspace()
    torch.cuda.synchronize()
    # what member 0's first step starts from besides its prognostics, for the anchor: the model's boundary fields and its qcorh
    start = {"bnd": dict({k: v.numpy()[0].reshape(-1) for k, v in bnd.items()}, albsfc=albsfc.numpy()[0].reshape(-1)),
             "qcorh": ens.qcorh[0].cpu().numpy(), "tyear": sm.Date(*er.DATE).tyear}

    def one(sw):
        ens.step(2, 2, dt, dict(P, sw=sw), eps=ROB)
        G.check_dev(ens.vor[1], ens.div[1], ens.t[1])
        M.couple_dev(1, *[F[k] for k in er.FLUXES])
    snaps, graphs = [], {}
    for n in range(RUN_STEPS):
        sw = n % 3 == 0
        if n == 1:
            M.forcing_dev(ens.qcorh)                     # the day's first step
        if graph:
            if sw not in graphs:
                with sp.graph_capture() as g:
                    one(sw)
                graphs[sw] = g
            graphs[sw].launch()
        else:
            one(sw)
        one_guard.check_dev(ens.vor[1, 1], ens.div[1, 1], ens.t[1, 1])
        sp.synchronize()
        snap = es.snapshot(ens)
        snap.update(rad=P["rad"].clone(), qcorh=ens.qcorh.clone(), surf={k: M.field(k).numpy() for k in er.SURF},
                    flux={k: F[k].clone() for k in er.FLUXES}, rows=np.stack([G.read(n, 1, member=e)[0] for e in range(E)]))
        snaps.append(snap)
        if inject and n + 1 == INJECT_AFTER:
            ens.t[1, 1] = complex(float("nan"), float("nan"))
            torch.cuda.synchronize()
    bad = (__import__("ctypes").c_longlong * E)()
    final = {"count": sp.lib.spdy_ens_diagnostics_stopped(G.h, bad), "stopped": list(bad), "status": [G.status(e) for e in range(E)],
             "single": one_guard.status(), "single_rows": one_guard.read(0, RUN_STEPS), "start": start}
    for g in graphs.values():
        g.close()
    M.close(); G.close(); one_guard.close()
    return snaps, final


def anchor_first_step(c, o, clean, start):
    """Member 0's first step of the clean run against the reference side of tests/test_gpu_coupled_run.py: the oracle's call-by-call
    step with the chain of restatements as its physics (physstep.Case.hook), on the member's state, the boundary fields and qcorh the
    surface model held before the step and the zonal forcing of the run's date.  Prognostics and PL operands within TOL."""
    import coupledrun
    sp, dt = c["sp"], c["dt"]
    st = dict(c["sts"][0], qcorh=start["qcorh"])
    case = physstep.Case("t30", sp, o, st=st, bnd=start["bnd"])
    case.zon = coupledrun.zonal(sp, case, start["tyear"])
    o.tail_init(dt)
    rec = {}
    new, out = oracle_dynamics_step(o, st, 2, dt, ROB, physics=case.hook(True, {}, rec))
    m = es.member_of(clean[0], 0)
    worst = synth.relerr(m["PL"].cpu().numpy(), out["PL"])
    assert worst <= TOL, ("PL", worst)
    for k in es.PROG:
        g = m[k].cpu().numpy()
        e = max(synth.relerr(g, new[k]), wave_relerr(g, new[k]))
        assert e <= TOL, (k, e)
        worst = max(worst, e)
    print("\n[coupled run] member 0, first step against the oracle with the restated physics: worst %.2e (smallest decision margin %.1e)"
          % (worst, float(rec["margin"].min())))


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_member_goes_nonfinite_in_a_coupled_run(graph, oracle_factory):
    """T30 L8, E = 3, the whole physics, a humidity correction per member, ONE surface model and ONE guard of three members, eight
    steps across a day boundary (forcing_dev), eager and as graph replays.  After the second step member 1's time-level-2
    temperature is overwritten with NaN.  After every later step members 0 and 2 are bit-equal to the clean run -- prognostics, phi,
    operands, flux outputs, surface-model fields, qcorh, radiation-state slices, guard rows -- and are not stopped; the guard
    reports member 1 with DIAG_NONFINITE from the first step whose check saw the NaN, with the level and the saved row that a
    single Diagnostics object on member 1's slice reports; one member counts as stopped.  The clean run stays finite and in range
    and member 0's first step is anchored to the oracle with the restated physics (anchor_first_step).  The members are the
    reference's rest state with a different seeded wind each (member 0 and 1: the states of the coupled three-day run), not the
    seeded states of the other parts: those are not balanced and overflow within three steps with the physics at any but a very short
    time step (tests/physstep.py, DT), and eight steps at the model's own 2400 s are what this test is about."""
    import ensemblerun as er
    c = coupled_setup(oracle_factory)
    sp, E = c["sp"], len(c["sts"])
    size = sp.radiation_state_size()
    if ("clean", graph) not in c["runs"]:
        c["runs"]["clean", graph] = coupled_run(c, False, graph)
    clean, clean_final = c["runs"]["clean", graph]
    assert clean_final["count"] == 0 and clean_final["stopped"] == [-1] * E, clean_final
    assert all(not poison.nonfinite(clean[-1][k]) for k in es.PROG) and np.isfinite(clean[-1]["rows"]).all()
    assert not support.same_bits(clean[-1]["vor"][:, 0], clean[-1]["vor"][:, 2])
    anchor_first_step(c, oracle_factory("t30"), clean, clean_final["start"])
    got, final = coupled_run(c, True, graph)
    first_bad = INJECT_AFTER                 # the guard's number (from 0) of the first step that starts from the NaN
    for n in range(RUN_STEPS):
        for e in (0, 2):
            a, b = es.member_of(got[n], e), es.member_of(clean[n], e)
            bad = [k for k in es.COMPARED if not support.same_bits(a[k], b[k])]
            bad += [k for k in ("qcorh",) if not support.same_bits(got[n][k][e], clean[n][k][e])]
            bad += ["flux " + k for k in er.FLUXES if not support.same_bits(got[n]["flux"][k][e], clean[n]["flux"][k][e])]
            bad += ["rad"] if not support.same_bits(got[n]["rad"][e * size:(e + 1) * size], clean[n]["rad"][e * size:(e + 1) * size]) else []
            bad += [k for k in er.SURF if not support.same_bits(got[n]["surf"][k][e], clean[n]["surf"][k][e])]
            bad += ["guard row"] if not support.same_bits(got[n]["rows"][e], clean[n]["rows"][e]) else []
            assert bad == [], "step %d (from 1), member %d differs from the clean run in %s" % (n + 1, e, bad)
        if n >= first_bad:
            assert poison.nonfinite(got[n]["t"][:, 1]), n
            assert not np.isfinite(got[n]["rows"][1]).all(), n
    assert final["count"] == 1 and final["stopped"] == [-1, first_bad, -1], final
    st, one = final["status"][1], final["single"]
    assert st["bad_mask"] & dg.NONFINITE and st["bad_step"] == first_bad == one["bad_step"], (st, one)
    assert st["bad_level"] == one["bad_level"] and st["bad_mask"] == one["bad_mask"], (st, one)
    assert support.same_bits(np.asarray(st["bad_row"]), np.asarray(one["bad_row"]))
    assert support.same_bits(np.stack([x["rows"][1] for x in got]), final["single_rows"])
    for e in (0, 2):
        assert final["status"][e]["bad_step"] == -1 and final["status"][e]["bad_mask"] == 0, (e, final["status"][e])
    assert poison.nonfinite(got[-1]["surf"]["stl_lm"][1]) and not poison.nonfinite(got[-1]["surf"]["stl_lm"][0])
