"""GPU: every host-pointer entry point of the C ABI (the cases of tests/hostcalls.py), through the one staging helper they share
(csrc/spdy_plan.hpp, spdy_detail::HostCall): both staging routes give the same bits, those are the bits of the `_dev` form, a call
of nothing writes nothing, and a refused call leaves nothing behind for the next one.

T30 and T63, kx = 8, max_batch = 16; nb = 0, 1, 3, 16 (nlev = 1, 8).  At the default threshold of 512 KB a buffer: a T30 grid is
36 864 B (13 fit, 16 do not), a T63 grid 147 456 B (3 fit, 4 do not), 16 T30 spectra of 15 872 B fit and 16 T63 spectra of
66 560 B do not -- so the default plan takes both routes at either resolution, for grid-sized and for spectrum-sized calls."""
import os
import subprocess
import sys

import numpy as np
import pytest

import hostcalls as hc
import support
from conftest import ROOT

pytestmark = pytest.mark.gpu
TAGS = ("t30", "t63")
GUARD = 64


@pytest.fixture(scope="module")
def plans():
    """(plan, its inputs) per (tag, route), made in the route's environment (the pattern of test_host_staging_routes_agree)"""
    def make(tag, route):
        with pytest.MonkeyPatch.context() as mp:
            mp.delenv("SPDY_HOST_STAGE_KB", raising=False)
            if hc.ROUTES[route] is not None:
                mp.setenv("SPDY_HOST_STAGE_KB", hc.ROUTES[route])
            sp = hc.plan(tag)
        return sp, hc.Data(sp)
    support.package()
    with support.plan_cache(make, plan_of=lambda made: made[0]) as get:
        yield get


@pytest.fixture(scope="module")
def host_results(plans):
    """(tag, route, case, nb) -> the outputs of the host-pointer call, computed once and left unchanged"""
    done = {}

    def get(tag, route, case, nb):
        key = (tag, route, case, nb)
        if key not in done:
            sp, d = plans(tag, route)
            rc, outs = hc.run_host(sp, case, hc.arguments(case, d, nb))
            assert rc == hc.OK, (key, rc)
            done[key] = outs
        return done[key]
    return get


def same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("case", sorted(hc.CASES))
@pytest.mark.parametrize("tag", TAGS)
def test_routes_agree(tag, case, host_results):
    """the device-staging route (SPDY_HOST_STAGE_KB=0) and the default plan, where small calls are host-mapped: the same bits in
    every output array at every size, the entries a call leaves untouched included"""
    for nb in hc.sizes(case):
        assert same(host_results(tag, "device", case, nb), host_results(tag, "default", case, nb)), nb


@pytest.mark.parametrize("case", sorted(c for c in hc.CASES if c not in hc.STAGES))
@pytest.mark.parametrize("tag", TAGS)
def test_equals_dev_form(tag, case, plans, host_results):
    """the `_dev` counterpart on device copies of the same arrays, the pre-filled outputs among them: bit for bit what the
    host-pointer form returns"""
    sp, d = plans(tag, "default")
    for nb in hc.sizes(case):
        rc, outs = hc.run_dev(sp, case, hc.arguments(case, d, nb))
        assert rc == hc.OK
        assert same(outs, host_results(tag, "default", case, nb)), nb


@pytest.mark.parametrize("tag", TAGS)
def test_stage_chains_equal_dev_transforms(tag):
    """the four stage calls have no `_dev` form: on the four-kernel path the transforms' `_dev` forms are their chains, kernel for
    kernel -- fourier_inv(legendre_inv(s)) is spec_to_grid_dev(s) and legendre_dir(fourier_dir(g)) is grid_to_spec_dev(g), bit for bit"""
    import torch
    sp = hc.plan(tag)
    sp.set_fused(0)
    d = hc.Data(sp)
    for nb in hc.BATCHES[1:]:
        g = torch.full((nb,) + sp.grid_shape, hc.FILL, dtype=torch.float64, device="cuda")
        s = torch.full((nb,) + sp.spec_shape, hc.FILL * (1 + 1j), dtype=torch.complex128, device="cuda")
        sp.spec_to_grid_dev(support.dev(d.S[:nb]), g, kcos=2)
        sp.grid_to_spec_dev(support.dev(d.G[:nb]), s)
        torch.cuda.synchronize()
        assert np.array_equal(sp.fourier_inv(sp.legendre_inv(d.S[:nb]), 2), g.cpu().numpy()), nb
        assert np.array_equal(sp.legendre_dir(sp.fourier_dir(d.G[:nb])), s.cpu().numpy()), nb
    sp.close()


@pytest.mark.parametrize("route", sorted(hc.ROUTES))
@pytest.mark.parametrize("tag", TAGS)
def test_nothing_in_nothing_out(tag, route, plans):
    """nb = 0, with arrays of one field so that a write would show: the call returns 0 and every output keeps what it was handed in
    with"""
    sp, d = plans(tag, route)
    for case in sorted(c for c in hc.CASES if 0 in hc.sizes(c)):
        args = hc.arguments(case, d, 1)
        before = [a.a.copy() for a in args if isinstance(a, hc.O)]
        rc, outs = hc.run_host(sp, case, [0] + args[1:])
        assert rc == hc.OK and same(outs, before), case


def guarded_spec_to_grid(sp, d):
    """a one-field spec_to_grid into the middle of a fresh array: (return code, the grid, whether the guards on either side kept
    their pattern)"""
    import ctypes
    n = sp.il * sp.ix
    buf = np.full(n + 2 * GUARD, -7.25)
    rc = sp.lib.spdy_spec_to_grid(sp.h, d.S[7].ctypes.data_as(ctypes.c_void_p), 1, ctypes.c_void_p(buf.ctypes.data + 8 * GUARD))
    return rc, buf[GUARD:GUARD + n].reshape(sp.grid_shape), bool(np.all(buf[:GUARD] == -7.25) and np.all(buf[GUARD + n:] == -7.25))


@pytest.mark.parametrize("tag", TAGS)
def test_refusals_leave_nothing_behind(tag, plans):
    """Every entry point refuses a null required pointer and nb = max_batch + 1 with SPDY_ERR_ARG, and any call inside an open
    capture with SPDY_ERR_STATE; the capture still ends cleanly.  The host-staged call made right after each refusal returns the
    bits a fresh plan returns and writes nowhere but into its own output."""
    import torch
    sp, d = plans(tag, "default")
    fresh = hc.plan(tag)
    rc, want, clean = guarded_spec_to_grid(fresh, d)
    fresh.close()
    assert rc == hc.OK and clean

    def next_call_is_sound(why):
        rc, got, clean = guarded_spec_to_grid(sp, d)
        assert rc == hc.OK and clean and np.array_equal(got, want), why

    for case in sorted(hc.CASES):
        sized = hc.CASES[case][0] is not None
        args = hc.arguments(case, d, 1)
        narrays = sum(isinstance(a, hc.I) for a in args)
        for k in (k for k in range(narrays) if k not in hc.OPTIONAL.get(case, ())):
            assert hc.run_host(sp, case, args, null=k)[0] == hc.ERR_ARG, (case, k)
            next_call_is_sound((case, "null", k))
        if sized:
            assert hc.run_host(sp, case, [hc.MAX_BATCH + 1] + args[1:])[0] == hc.ERR_ARG, case
            next_call_is_sound((case, "nb"))
    # inside an open capture: every call is refused, a _dev call is recorded, and the capture ends with a graph that replays
    t = support.dev(d.S[:1])
    sp.use_own_stream()
    with sp.graph_capture() as g:
        for case in sorted(hc.CASES):
            assert hc.run_host(sp, case, hc.arguments(case, d, 1))[0] == hc.ERR_STATE, case
        assert sp.lib.spdy_trunct_dev(sp.h, 1, t.data_ptr()) == hc.OK
    g.launch()
    sp.synchronize()
    g.close()
    sp.use_torch_stream()
    torch.cuda.synchronize()
    next_call_is_sound("capture")


@pytest.mark.parametrize("route", sorted(hc.ROUTES))
def test_without_the_spin(route, plans):
    """SPDY_HOST_SPIN=0 (read once per process, hence a child): a T30 one-field round trip ends in the stream's synchronisation and
    gives the bits it gives with the spin, on either route"""
    sp, d = plans("t30", route)
    env = dict(os.environ, SPDY_HOST_SPIN="0")
    env.pop("SPDY_HOST_STAGE_KB", None)
    if hc.ROUTES[route] is not None:
        env["SPDY_HOST_STAGE_KB"] = hc.ROUTES[route]
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "hostcalls.py")], env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stdout.split()[-1] == hc.round_trip(sp, d)


