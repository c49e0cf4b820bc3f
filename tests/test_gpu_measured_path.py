"""GPU: the path bench.py times, checked -- throughput-sized batches on the plan's own stream, captured as one HIP graph, with the
streaming (non-temporal) store routes, against the C oracle field by field.

  * test_bench_dump_matches_reference: bench.py itself (a child process) and what its last timed step computed (--dump-outputs).
  * test_chained_round_trips_graph: K round trips in one graph sharing one spectra buffer, inputs that differ per step and that
    change in place between replays -- an overlapped or stale read at a launch boundary gives wrong fields here, where bench's
    fixed-input step would still read the right values.
  * test_route_handoffs_in_one_graph: producer and consumer launches on different store routes (streaming, resident, by-part,
    split, staged, by-chunk written through) in one graph, each consumer reading a slice of an earlier launch's output.
  * test_composite_guarded: the composite entry points at odd sizes and one size past each launch threshold.

Every output is a view into a larger allocation with sentinel fields around it (tests/guards.py) and starts as NaN; after every
eager run and every replay the sentinels must be bit-unchanged and the inputs equal to copies taken before.  The bar is TOL per
field (synth.relerr of each field), not per array.  Where the inputs are bench's tiled templates times a per-field scale, the
reference of a field is the oracle's result for its template times that scale (linearity), so every field is checked.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import synth
from conftest import ROOT, TOL
from guards import GRID_BYTES, STREAM_MIN, WT_MIN, Guarded, field_err, max_wg, pin_launch_options, route, worst

pytestmark = pytest.mark.gpu

NB = {"t30": 6144, "t63": 1536}          # bench.py's batch per GPU
DIMS = {"t30": (30, 96, 48), "t63": (63, 192, 96)}    # trunc, ix, il
UNIQ = 64                                # templates tiled over the batch (bench.headline_grids)
BENCH_TIMEOUT = 300                      # seconds for one bench.py child run (about 20-40 s on an MI355X)


def num_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def own_plan(tag, max_batch, fused=-1):
    """A plan on its own stream, like bench.py's, with the launch options at their defaults."""
    import speedy_f90_amd as s
    sp = s.Spectral(tag, kx=8, max_batch=max_batch, device=0)
    sp.use_own_stream()
    sp.set_fused(fused)
    pin_launch_options(sp)
    return sp


def assert_fields(name, got, ref, tol=TOL):
    """Every field of `got` within tol of `ref` (device tensors, leading axis = field); returns the worst error."""
    import torch
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err = field_err(torch, got, ref)
    i, e = worst(err)
    bad = np.flatnonzero(~(err <= tol))
    assert bad.size == 0, "%s: %d of %d fields over %g (NaN counts), first %s, worst field %d: %r" % (
        name, bad.size, err.size, tol, bad[:8].tolist(), i, e)
    return e


def assert_guards(label, guards):
    for name, g in guards.items():
        assert g.intact(), "%s: sentinel fields of %s overwritten at (band, field) %s" % (label, name, g.hits()[:8])


def assert_inputs(label, inputs, copies):
    import torch
    for i, (a, c) in enumerate(zip(inputs, copies)):
        assert torch.equal(a, c), "%s: input %d changed" % (label, i)


def oracle_stack(fn, xs):
    """The oracle applied to each field of the host array xs, one field at a time, as a stacked NumPy array."""
    return np.stack([fn(x) for x in xs])


_TEMPLATES = {}


def templates(tag, oracle_factory):
    """bench.headline_grids' 64 templates on the device with their references: (T, g2s(T), s2g(g2s(T), 1))."""
    import torch
    if tag not in _TEMPLATES:
        o = oracle_factory(tag)
        _, ix, il = DIMS[tag]
        T = synth.grids(UNIQ, ix, il, first=0)
        RS = oracle_stack(o.grid_to_spec, T)
        RG = oracle_stack(lambda x: o.spec_to_grid(x, 1), RS)
        _TEMPLATES[tag] = tuple(torch.from_numpy(a).cuda() for a in (T, RS, RG))
    return _TEMPLATES[tag]


def scales(seed, nb):
    """A seeded scale in [0.5, 1.5) per field, as a device column for broadcasting over a field."""
    import torch
    return torch.from_numpy(0.5 + synth.splitmix64(seed, nb)).cuda()


def tiled(t, s):
    """Template i % 64 times s[i] for every field i (the shape of bench's input)."""
    nb = s.shape[0]
    return t.repeat((nb + UNIQ - 1) // UNIQ, *([1] * (t.dim() - 1)))[:nb] * s.view((nb,) + (1,) * (t.dim() - 1))


def pick_odd(lo, hi, want):
    """An odd size in [lo, hi], as close to `want` as the range allows."""
    assert lo <= hi, "no size between %d and %d on this device" % (lo, hi)
    n = min(max(want, lo), hi) | 1
    return n if n <= hi else n - 2


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------------- 1. bench's own outputs
def _tail(out, err, n=3000):
    dec = lambda b: b.decode(errors="replace") if isinstance(b, bytes) else (b or "")
    return ("stdout:\n" + dec(out)[-n:] + "\nstderr:\n" + dec(err)[-n:])


@pytest.mark.parametrize("res", ["t30", "t63"])
def test_bench_dump_matches_reference(res, tmp_path, oracle_factory):
    """bench.py as a child process, its timed graph replays at the full batch, and what the last timed step computed
    (--dump-outputs) against the oracle: every dumped field of both transforms, and the direct output's structural zeros."""
    import torch
    import bench
    out = str(tmp_path / "dump")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--res", res, "--steps", "20", "--warmup", "2", "--no-extras",
           "--no-cpu-baseline", "--no-pmc", "--no-multi", "--dump-outputs", out]
    try:
        run = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=BENCH_TIMEOUT)
    except subprocess.TimeoutExpired as e:
        pytest.fail("bench.py did not finish in %d s\n%s" % (BENCH_TIMEOUT, _tail(e.stdout, e.stderr)))
    if run.returncode != 0:
        pytest.fail("bench.py exited with status %d\n%s" % (run.returncode, _tail(run.stdout, run.stderr)))
    lines = run.stdout.strip().splitlines()
    assert lines, _tail(run.stdout, run.stderr)
    line = json.loads(lines[-1])
    assert line["value"] > 0 and "dump_outputs" in line, lines[-1][:2000]
    dumped = line["dump_outputs"]

    o = oracle_factory(res)
    nb = NB[res]

    trunc, ix, il = DIMS[res]

    class Stub:                                                  # all headline_grids reads of the plan
        pass
    Stub.ix, Stub.il = ix, il
    grid = bench.headline_grids(torch, synth, Stub, nb, 0, "cpu").numpy()
    gts = np.load(os.path.join(out, "grid_to_spec.npy"))
    stg = np.load(os.path.join(out, "spec_to_grid.npy"))
    # the dumped fields, exactly as bench.dump_outputs picks them (one rank)
    per_field = (il * ix + 2 * (trunc + 2) * (trunc + 1)) * 8
    n = min(nb, bench.DUMP_BYTES // per_field)
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(nb, n, replace=False)) if n < nb else np.arange(nb)
    assert n == dumped["fields"] and dumped["of_fields"] == nb, (n, dumped)
    assert gts.shape[0] == n and stg.shape[0] == n
    spec = gts[..., 0] + 1j * gts[..., 1]
    assert spec.shape[1:] == (trunc + 2, trunc + 1) and stg.shape[1:] == (il, ix)
    e_dir = np.array([synth.relerr(spec[j], o.grid_to_spec(grid[b])) for j, b in enumerate(idx)])
    e_inv = np.array([synth.relerr(stg[j], o.spec_to_grid(spec[j], 1)) for j in range(n)])
    for name, e in (("grid_to_spec", e_dir), ("spec_to_grid", e_inv)):
        bad = np.flatnonzero(~(e <= TOL))
        assert bad.size == 0, "%s: fields %s of the dump over %g (worst %r)" % (name, idx[bad[:8]].tolist(), TOL, worst(e))
    # structural zeros of the direct output: row nx, l > trunc + 1, Im(m' = 0)
    l = np.add.outer(np.arange(spec.shape[1]), np.arange(spec.shape[2]))
    assert np.all(spec[:, -1, :] == 0)
    assert np.all(spec[:, l > trunc + 1] == 0)
    assert np.all(spec[:, :, 0].imag == 0)
    print("\n[%s] bench dump: %d of %d fields, worst grid_to_spec %.2e, spec_to_grid %.2e; %s, %.4g round trips/s"
          % (res, n, nb, worst(e_dir)[1], worst(e_inv)[1], line.get("timed_launch"), line["value"]))


# ------------------------------------------------------------------------------------- 2. chained steps, inputs that change
K = 3


@pytest.mark.parametrize("tag,fused,in_place", [("t30", -1, False), ("t30", 0, False), ("t63", -1, False), ("t63", 0, False),
                                                ("t30", -1, True), ("t30", 0, True), ("t63", -1, True), ("t63", 0, True)],
                         ids=["t30-auto", "t30-four", "t63-auto", "t63-four",
                              "t30-auto-in_place", "t30-four-in_place", "t63-auto-in_place", "t63-four-in_place"])
def test_chained_round_trips_graph(tag, fused, in_place, oracle_factory):
    """K round trips captured in one graph on the plan's own stream.  Step k reads its own grids G_k and writes its own O_k
    (in_place: back over G_k, bench's round_trip_in_place); all steps share ONE spectra buffer, as bench's steps do, so a
    step k+1 direct transform that overwrites it while step k's inverse still reads it makes O_k wrong.  Between replays
    every G_k changes in place (a new seeded scale per field), so a value left from the previous replay is wrong too."""
    import torch
    nb = NB[tag]
    T, RS, RG = templates(tag, oracle_factory)
    sp = own_plan(tag, nb, fused)
    gshape, sshape = (sp.il, sp.ix), (sp.nx, sp.mx)
    # graph buffers and a second set for the eager runs; the direct transforms' shared spectra are guarded too
    sets = []
    for _ in range(2):
        if in_place:
            gg = Guarded(torch, gshape, [nb] * K)
            grids, outs, guards = gg.outs, gg.outs, {"grids": gg}
        else:
            go = Guarded(torch, gshape, [nb] * K)
            grids = [torch.empty((nb,) + gshape, dtype=torch.float64, device="cuda") for _ in range(K)]
            outs, guards = go.outs, {"outs": go}
        gs = Guarded(torch, sshape, [nb], complex_=True)
        guards["spec"] = gs
        sets.append((grids, outs, gs.outs[0], guards))

    def steps(grids, outs, spec):
        for k in range(K):
            sp.grid_to_spec_dev(grids[k], spec)
            sp.spec_to_grid_dev(spec, outs[k], kcos=1)

    g_grids, g_outs, g_spec, g_guards = sets[0]
    e_grids, e_outs, e_spec, e_guards = sets[1]
    torch.cuda.synchronize()
    with sp.graph_capture() as graph:
        steps(g_grids, g_outs, g_spec)
    torch.cuda.synchronize()
    assert all(bool(x.isnan().all()) for x in g_outs)                            # nothing ran during the capture
    worst_e = 0.0
    for rep in range(2):
        sc = [scales(9100 + 10 * rep + k, nb) for k in range(K)]
        for grids in (g_grids, e_grids):
            for k in range(K):
                grids[k].copy_(tiled(T, sc[k]))                                         # in place, on torch's stream
        torch.cuda.synchronize()
        refs = [tiled(RG, sc[k]) for k in range(K)]
        ref_spec = tiled(RS, sc[K - 1])
        for what, (grids, outs, spec, guards) in (("eager", sets[1]), ("replay", sets[0])):
            label = "%s %d" % (what, rep)
            copies = [] if in_place else [g.clone() for g in grids]
            torch.cuda.synchronize()
            if what == "eager":
                steps(grids, outs, spec)
            else:
                graph.launch()
            sp.synchronize()
            assert_guards(label, guards)
            assert_inputs(label, grids, copies)
            for k in range(K):
                worst_e = max(worst_e, assert_fields("%s: O_%d" % (label, k), outs[k], refs[k]))
            worst_e = max(worst_e, assert_fields("%s: shared spectra" % label, spec, ref_spec))
        for k in range(K):
            assert torch.equal(g_outs[k], e_outs[k]), "replay %d: O_%d differs from the eager run" % (rep, k)
        assert torch.equal(g_spec, e_spec), "replay %d: spectra differ from the eager run" % rep
    n = num_cu()
    print("\n[%s fused=%d in_place=%d] K=%d x B=%d, 2 replays: worst field error %.2e; routes g2s %s, s2g %s"
          % (tag, fused, in_place, K, nb, worst_e, route(tag, "g2s", nb, n, max_batch=nb) if fused else "four-kernel",
             route(tag, "s2g", nb, n) if fused else "four-kernel"))
    graph.close()
    sp.close()


# ----------------------------------------------------------------------------------- 3. producer / consumer route handoffs
def handoff_chain(tag, n_cu):
    """The launches of the route-handoff graph: (name, direction, source, first field of the slice, fields, kcos, route).
    Source "G" is the input grids, otherwise the output of the named earlier launch.  Sizes from the CU count:
      T30  part:     3 tiles per workgroup round fit: 3 ceil(n/2) <= wg;        resident: above that, under 16 MiB of grids
           split:    6 ceil(n/2) <= wg (direct)
      T63  chunk_wt: 2 ceil(n/2) <= CUs and n fields of grids >= 6 MiB;       staged: 3 ceil(n/2) <= CUs
           split:    2 ceil(n/2) <= CUs but not staged (3 ceil(n/2) > CUs)."""
    nb = NB[tag]
    gb = GRID_BYTES[tag]
    if tag == "t30":
        wg = max_wg(tag, n_cu)
        n_res = pick_odd(2 * (wg // 3) + 1, (STREAM_MIN - 1) // gb, 301)
        return [("D1", "g2s", "G", 0, nb, None, "stream"),
                ("I1", "s2g", "D1", 3001, 5, 2, "part"),
                ("D2", "g2s", "I1", 0, 5, None, "split"),
                ("I2", "s2g", "D1", 1, n_res, 1, "resident"),
                ("I3", "s2g", "D1", 0, nb, 1, "stream")]
    n_wt = pick_odd(-(-WT_MIN // gb), min(n_cu, (STREAM_MIN - 1) // gb), 61)
    n_split = pick_odd(2 * (n_cu // 3) + 1, 2 * (n_cu // 2), 201)
    return [("D1", "g2s", "G", 0, nb, None, "stream"),
            ("I1", "s2g", "D1", 501, n_wt, 2, "chunk_wt"),
            ("D2", "g2s", "I1", 0, 5, None, "staged"),
            ("I2", "s2g", "D1", 0, nb, 1, "stream"),
            ("D3", "g2s", "I2", 333, n_split, None, "split")]


@pytest.mark.parametrize("tag", ["t30", "t63"])
def test_route_handoffs_in_one_graph(tag, oracle_factory):
    """One graph whose launches take different store routes, each consumer reading a slice of an earlier launch's output:
    streaming direct -> by-part inverse -> split direct, and resident / streaming inverses of the first spectra (T30);
    streaming direct -> by-chunk written-through inverse -> staged direct, streaming inverse -> split direct (T63).
    Eager and replay bit-equal, every output field against the oracle applied to the device's own input of that launch."""
    import torch
    nb = NB[tag]
    n_cu = num_cu()
    chain = handoff_chain(tag, n_cu)
    for name, d, src, first, n, kc, want in chain:
        assert route(tag, d, n, n_cu, max_batch=nb) == want, (name, n, route(tag, d, n, n_cu, max_batch=nb), want)
    o = oracle_factory(tag)
    T, RS, RG = templates(tag, oracle_factory)
    sp = own_plan(tag, nb)
    gshape, sshape = (sp.il, sp.ix), (sp.nx, sp.mx)
    G = tiled(T, scales(9300, nb)).contiguous()
    ref_S1 = tiled(RS, scales(9300, nb))

    def buffers():
        out, guards = {}, {}
        for name, d, src, first, n, kc, want in chain:
            g = Guarded(torch, sshape if d == "g2s" else gshape, [n], complex_=d == "g2s")
            out[name], guards[name] = g.outs[0], g
        return out, guards

    def run(out):
        for name, d, src, first, n, kc, want in chain:
            x = (G if src == "G" else out[src])[first:first + n]
            if d == "g2s":
                sp.grid_to_spec_dev(x, out[name])
            else:
                sp.spec_to_grid_dev(x, out[name], kcos=kc)

    g_out, g_guards = buffers()
    e_out, e_guards = buffers()
    G0 = G.clone()
    torch.cuda.synchronize()
    with sp.graph_capture() as graph:
        run(g_out)
    torch.cuda.synchronize()
    run(e_out)
    sp.synchronize()
    assert_guards("eager", e_guards)
    assert_inputs("eager", [G], [G0])
    graph.launch()
    sp.synchronize()
    assert_guards("replay", g_guards)
    assert_inputs("replay", [G], [G0])
    report = []
    for name, d, src, first, n, kc, want in chain:
        assert torch.equal(g_out[name], e_out[name]), "%s (%s): replay differs from the eager run" % (name, want)
        got = g_out[name]
        if src == "G":
            ref = ref_S1                                         # the tiled templates: linearity
        else:
            x = g_out[src][first:first + n].cpu().numpy()        # the oracle on this launch's own input
            ref = to_dev(oracle_stack(o.grid_to_spec, x) if d == "g2s" else oracle_stack(lambda f: o.spec_to_grid(f, kc), x))
        e = assert_fields("%s (%s %s, %d fields from %s[%d:])" % (name, want, d, n, src, first), got, ref)
        report.append("%s %s %s n=%d: %.2e" % (name, d, want, n, e))
    print("\n[%s] %d CUs: %s" % (tag, n_cu, "; ".join(report)))
    graph.close()
    sp.close()


# --------------------------------------------------------------------------------- 4. composite entry points, odd sizes
def composite_sizes(tag, op, n_cu):
    """nb = 1, 3 and one size past each launch threshold of `op` (see guards.route and the launchers)."""
    gb = GRID_BYTES[tag]
    stream_pairs = -(-STREAM_MIN // (2 * gb))                    # pairs of grids from which a launch streams
    if tag == "t30":
        wg = max_wg(tag, n_cu)
        past = [wg // 3 + 1, stream_pairs] if op != "vdspec" else [wg // 6 + 1, stream_pairs]
    elif op != "vdspec":
        past = [2 * (n_cu // 24) + 1,                            # past derive-on-load (s2g_t63_derives: 2 x 2 ceil(n/2) x 6 <= CUs)
                -(-WT_MIN // (2 * gb)),                          # by-chunk, written through
                2 * (n_cu // 4) + 1]                             # past by-chunk: 2 x 2 ceil(n/2) > CUs
    else:
        past = [min(n_cu // 3, 129) + 1,                         # past staged (vds in the contraction)
                2 * (n_cu // 4) + 1]                             # past split
    return sorted({1, 3} | set(past))


COMPOSITE = [(tag, op) for tag in ("t30", "t63") for op in ("uvspec_to_grid", "grad_to_grid", "vdspec", "inverse_segs", "direct_batch")]


@pytest.mark.parametrize("tag,op", COMPOSITE, ids=["%s-%s" % c for c in COMPOSITE])
def test_composite_guarded(tag, op, oracle_factory):
    """The composite entry points with every output guarded: sentinels around and between the outputs of one call, outputs
    NaN-filled, inputs compared with copies -- at odd sizes (partial T30 tiles, odd T63 pairs) and one size past each launch
    threshold -- and every output field against the oracle's sequence of reference calls."""
    import torch
    o = oracle_factory(tag)
    n_cu = num_cu()
    sp = own_plan(tag, 512)
    gshape, sshape = (sp.il, sp.ix), (sp.nx, sp.mx)
    s2g = lambda kc: (lambda f: o.spec_to_grid(f, kc))
    report = []
    if op in ("uvspec_to_grid", "grad_to_grid", "vdspec"):
        cases = [(n,) for n in composite_sizes(tag, op, n_cu)]
    elif op == "inverse_segs":
        cases = [(3, (3, 5, 1, 7), 3), (1, (1,), 0), (5, (7, 2), 5)]            # (pairs, plain segments, gradients)
    else:
        stream_fields = -(-STREAM_MIN // GRID_BYTES[tag])
        cases = [(3, 5), (1, 1), (0, 7), (3, stream_fields - 6 + 1)]          # (pairs, plain): the last one past one mixed launch
    for case in cases:
        nb = case[0]
        inputs, outs, refs = [], None, []
        if op in ("uvspec_to_grid", "grad_to_grid"):
            S = synth.spectra(2 * nb, sp.trunc, first=5100 + nb, full_rows=True)
            vor, div = to_dev(S[:nb]), to_dev(S[nb:])
            g = Guarded(torch, gshape, [nb, nb])
            if op == "uvspec_to_grid":
                inputs = [vor, div]
                call = lambda: sp.uvspec_to_grid_dev(vor, div, g.outs[0], g.outs[1], 2)
                uv = [o.uvspec(S[b], S[nb + b]) for b in range(nb)]
            else:
                inputs = [vor]
                call = lambda: sp.grad_to_grid_dev(vor, g.outs[0], g.outs[1], 2)
                uv = [o.grad(S[b]) for b in range(nb)]
            refs = [np.stack([s2g(2)(u[0]) for u in uv]), np.stack([s2g(2)(u[1]) for u in uv])]
            guards = {"out": g}
        elif op == "vdspec":
            Gh = synth.grids(2 * nb, sp.ix, sp.il, first=5200 + nb)
            ug, vg = to_dev(Gh[:nb]), to_dev(Gh[nb:])
            g = Guarded(torch, sshape, [nb, nb], complex_=True)
            inputs = [ug, vg]
            call = lambda: sp.vdspec_dev(ug, vg, g.outs[0], g.outs[1], 2)
            vd = [o.vdspec(Gh[b], Gh[nb + b], 2) for b in range(nb)]
            refs = [np.stack([v[0] for v in vd]), np.stack([v[1] for v in vd])]
            guards = {"out": g}
        elif op == "inverse_segs":
            npairs, segs, ngrad = case
            nplain = sum(segs)
            S = synth.spectra(2 * npairs + nplain + ngrad, sp.trunc, first=5300 + nplain, full_rows=True)
            vor, div = to_dev(S[:npairs]), to_dev(S[npairs:2 * npairs])
            at, specs = 2 * npairs, []
            for n in segs:
                specs.append(to_dev(S[at:at + n]))
                at += n
            psi = to_dev(S[at:at + ngrad]) if ngrad else None
            counts = [npairs, npairs, nplain] + ([ngrad, ngrad] if ngrad else [])
            g = Guarded(torch, gshape, counts)
            go = g.outs
            inputs = [vor, div] + specs + ([psi] if ngrad else [])
            call = lambda: sp.inverse_batch_segs_dev(vor, div, go[0], go[1], specs, go[2], psi, go[3] if ngrad else None,
                                                     go[4] if ngrad else None, kcos_pairs=2, kcos=1, kcos_grad=2)
            uv = [o.uvspec(S[b], S[npairs + b]) for b in range(npairs)]
            refs = [np.stack([s2g(2)(u[0]) for u in uv]), np.stack([s2g(2)(u[1]) for u in uv]),
                    oracle_stack(s2g(1), S[2 * npairs:2 * npairs + nplain])]
            if ngrad:
                gr = [o.grad(S[at + b]) for b in range(ngrad)]
                refs += [np.stack([s2g(2)(x[0]) for x in gr]), np.stack([s2g(2)(x[1]) for x in gr])]
            guards = {"out": g}
        else:
            npairs, nplain = case
            Gh = synth.grids(2 * npairs + nplain, sp.ix, sp.il, first=5400 + nplain)
            ug, vg, gp = to_dev(Gh[:npairs]), to_dev(Gh[npairs:2 * npairs]), to_dev(Gh[2 * npairs:])
            g = Guarded(torch, sshape, [npairs, npairs, nplain] if npairs else [1, 1, nplain], complex_=True)
            vor, dv, spec = g.outs
            inputs = [ug, vg, gp]
            call = lambda: sp.direct_batch_dev(ug, vg, vor, dv, gp, spec, 2)
            vd = [o.vdspec(Gh[b], Gh[npairs + b], 2) for b in range(npairs)]
            refs = ([np.stack([v[0] for v in vd]), np.stack([v[1] for v in vd])] if npairs else [None, None])
            refs.append(oracle_stack(o.grid_to_spec, Gh[2 * npairs:]))
            guards = {"out": g}
        copies = [x.clone() for x in inputs]
        torch.cuda.synchronize()
        call()
        sp.synchronize()
        label = "%s %s %s" % (tag, op, case)
        assert_guards(label, guards)
        assert_inputs(label, inputs, copies)
        e = 0.0
        for i, (got, ref) in enumerate(zip(g.outs, refs)):
            if ref is None:                                      # (no pairs: the unused pair outputs stay NaN, untouched)
                assert bool(got.isnan().all()), "%s: output %d written without pairs" % (label, i)
                continue
            e = max(e, assert_fields("%s output %d" % (label, i), got, to_dev(ref)))
        if op in ("uvspec_to_grid", "grad_to_grid", "vdspec"):
            report.append("n=%d %s: %.2e" % (nb, route(tag, "g2s" if op == "vdspec" else "s2g", nb, n_cu, pairs=True, max_batch=512), e))
        else:
            report.append("%s: %.2e" % (case, e))
    print("\n[%s %s] %d CUs: %s" % (tag, op, n_cu, "; ".join(report)))
    sp.close()
