"""CPU: host logic of the product -- C-ABI surface, table generation, loud failure without a GPU."""
import ctypes
import os

import numpy as np
import pytest

import support
import synth
from conftest import ROOT
from support import pkg  # noqa: F401

TAGS = ("t30", "t63")


def test_cabi_exports_every_declared_symbol(pkg):
    """include/spdy.h is the contract: every function it declares must be exported and bound."""
    declared = support.declared()
    assert len(declared) >= 35
    lib = ctypes.CDLL(pkg.LIB_PATH)
    for name in sorted(declared):
        assert hasattr(lib, name), "missing export " + name
    from importlib import import_module
    sigs = import_module("speedy_f90_amd._lib").SIGNATURES
    assert declared - {"spdy_last_error"} == set(sigs), "python binding and header disagree"
    # nothing leaks except the C ABI
    out = os.popen("nm -D --defined-only %s" % pkg.LIB_PATH).read()
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert {e for e in exported if e.startswith("spdy_")} == declared


@pytest.mark.parametrize("tag", TAGS)
def test_product_tables_match_oracle(tag, pkg, oracle_factory):
    """Product table generation (csrc/spdy_tables.cpp) is an independent implementation of the
    reference recipes; it must agree with the oracle bit for bit (both are plain IEEE)."""
    sp = pkg.Spectral(tag, device=-1)
    o = oracle_factory(tag)
    names = ["sia_half", "cosgr", "cosgr2", "hsg", "dhs", "fsg", "dhsr", "fsgr", "work", "ifac", "epsi", "wt",
             "poly", "nsh2", "el2", "elm2", "el4", "trfilt", "gradx", "gradyp", "uvdx", "uvdym", "uvdyp",
             "vddym", "vddyp", "dmp", "dmpd", "dmps"]
    for n in names:
        assert np.array_equal(sp.table(n), o.table(n)), n
    assert np.array_equal(sp.table("gradym").reshape(o.nx, o.mx)[1:], o.table("gradym").reshape(o.nx, o.mx)[1:])
    assert np.array_equal(sp.table("coa_half")[: o.iy], o.table("coa_half")[: o.iy])
    for dt in (1200.0, 4800.0):
        sp.initialize_implicit(dt)
        o.tail_init(dt)
        for n in ("dmp1", "dmp1d", "dmp1s", "tref", "tref1", "tref2", "tref3", "xc", "xd", "xj", "dhsx", "elz"):
            assert np.array_equal(sp.table(n), o.table(n)), (dt, n)


@pytest.mark.parametrize("tag", TAGS)
def test_product_tables_match_golden(tag, pkg, golden):
    sp = pkg.Spectral(tag, device=-1)
    g = golden(tag)
    for n in ("sia_half", "cosgr", "cosgr2", "hsg", "dhs", "fsg", "dhsr", "fsgr", "work"):
        assert np.array_equal(sp.table(n), g["tab_" + n]), n
    assert np.array_equal(sp.table("epsi"), g["tab_epsi"].ravel())
    assert np.array_equal(sp.table("el2"), g["tab_el2"].ravel())
    sp.initialize_implicit(4800.0)
    for n in ("dmp", "dmpd", "dmps", "dmp1", "dmp1d", "dmp1s", "tref", "tref2", "tref3"):
        assert np.array_equal(sp.table(n), g["dt4800_" + n].ravel()), n


def test_no_cpu_fallback(pkg):
    """Without a device every compute entry point fails loudly (SPDY_ERR_NO_DEVICE)."""
    sp = pkg.Spectral("t30", device=-1)
    with pytest.raises(pkg.SpdyError) as e:
        sp.grid_to_spec(np.zeros(sp.grid_shape))
    assert e.value.code == -3
    with pytest.raises(pkg.SpdyError):
        sp.spec_to_grid(np.zeros(sp.spec_shape, np.complex128))
    with pytest.raises(pkg.SpdyError):
        sp.uvspec(np.zeros(sp.spec_shape, np.complex128), np.zeros(sp.spec_shape, np.complex128))
    try:
        import torch
        has_gpu = torch.cuda.is_available()
    except Exception:
        has_gpu = False
    if not has_gpu:
        with pytest.raises(pkg.SpdyError) as e:
            pkg.Spectral("t30", device=0)
        assert e.value.code == -3


def test_argument_errors(pkg):
    with pytest.raises(pkg.SpdyError) as e:
        pkg.Spectral((21, 64, 16), device=-1)
    assert e.value.code == -2                       # unsupported resolution
    with pytest.raises(pkg.SpdyError):
        pkg.Spectral("t30", max_batch=0, device=-1)
    sp = pkg.Spectral("t30", kx=6, device=-1)
    with pytest.raises(pkg.SpdyError):              # no sigma levels for kx=6 (geometry.f90:42-48)
        sp.initialize_implicit(2400.0)
    with pytest.raises(pkg.SpdyError):
        sp.table("no_such_table")
    with pytest.raises(ValueError):
        sp.grid_to_spec(np.zeros((3, 3)))


def test_product_does_not_touch_oracle():
    """The product tree must not reference oracle/ in any form."""
    pk = os.path.join(ROOT, "speedy.f90_amd")
    for dirpath, _, files in os.walk(pk):
        if os.path.basename(dirpath) in ("build", "__pycache__"):
            continue
        for f in files:
            if f.endswith((".py", ".cpp", ".hpp", ".hip", ".inc", ".h", ".f90", "Makefile")):
                txt = open(os.path.join(dirpath, f), errors="replace").read()
                assert "oracle" not in txt.lower().replace("oracle/ in any form", ""), os.path.join(dirpath, f)


def test_synth_reproducible():
    a = synth.splitmix64(20240229, 4)
    assert np.allclose(a, synth.splitmix64(20240229, 4))
    s = synth.spectra(2, 30)
    assert s.shape == (2, 32, 31) and np.all(s[:, :, 0].imag == 0) and np.all(s[:, 31, :] == 0)
    assert np.all(s[0][np.add.outer(np.arange(32), np.arange(31)) > 30] == 0)


def test_bench_launches_its_own_ranks():
    """`python bench.py --gpus N` with no launcher environment starts N ranks itself (torch.distributed.run, rendezvous on
    127.0.0.1): --dry-launch makes every rank print the environment it was given and exit, so this runs without a GPU."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "3", "--dry-launch"], env=env,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    ranks = [json.loads(ln) for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert sorted(r["rank"] for r in ranks) == [0, 1, 2]
    assert sorted(r["local_rank"] for r in ranks) == [0, 1, 2]
    assert all(r["world_size"] == 3 and r["master_addr"] == "127.0.0.1" and r["hsa_ipc_legacy"] == "0" for r in ranks)
    # a launcher that started a different number of ranks than --gpus asks for is refused (never "n_gpus": 1 for --gpus 8)
    bad = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "8", "--dry-launch"],
                         env=dict(env, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0"), capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and "WORLD_SIZE=1" in bad.stderr


def test_bench_force_multi_needs_full():
    """--force-multi asks for a side measurement, which only a --full run makes: without --full it is refused before any
    GPU work (so this runs without a GPU)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--force-multi"], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode != 0 and "--full" in out.stderr


def test_no_store_data_hazard_in_isa():
    """Static check of the compiled gfx950 kernels (tools/scan_store_hazard.py): no vector-memory store of more than 64 bits has
    one of its data registers rewritten within two wait states.  On gfx950 such a store still reads the last lanes of every 16-lane
    row when the next instructions issue; the compiler inserts one wait state (none for a buffer store with an SGPR soffset), and
    tools/store_valu_hazard.hip shows one is not enough.  The T63 inverse kernel had 19 such pairs until the end of round 3
    (dormant with its roles on separate SIMDs, wrong values with them mixed: DESIGN s4.3)."""
    import shutil
    import subprocess
    import sys
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("no hipcc here")
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "scan_store_hazard.py")
    r = subprocess.run([sys.executable, tool], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr



def test_bench_collects_errors_of_side_measurements():
    """bench.py lists every failed side measurement by path in a top-level `errors` entry (round 4's driver run carried a nested
    RuntimeError string nobody saw)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_for_test", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    res = {"value": 1.0, "extras": {"a": {"error": "RuntimeError('x')"}, "b": [{"ok": 1}, {"error": "y"}], "c": {"fine": True}}, "errors": []}
    got = bench.collect_errors(res)
    assert [e["where"] for e in got] == ["extras.a", "extras.b[1]"]
    assert bench.collect_errors({"extras": {"c": {"fine": True}}}) == []
