"""Level counts of the column physics outside support.PHYSICS_TAGS: one count per class of the column kernels' two instantiations
(csrc/spdy_columns.hpp launch_columns: <8> for kx <= 8, <16> for kx <= 16), on tests/levels.py's half levels at T30.

    kx     instantiation   what the count is
    6      <8>             the free count of <8>: two unused levels; the first count at which do k = kx-3, 3, -1 of the convection
                           diagnosis (convection.f90:213) runs at all -- once, at k = 3
    9      <16>            first of <16>: seven unused levels
    12     <16>            the middle of the class, even
    15     <16>            one short of full: a single unused level

support.PHYSICS_TAGS has 5, 7, 8 (<8>) and 16 (<16> with k < kx the same as k < KMAX).  The variants here are named "t30k<kx>"; they are not in
conftest.VARIANTS, and their fixture is tests/golden/ref_physlevels.npz (tests/golden/make_golden_physlevels.py)."""
import levels
import moist
import support

COUNTS = (6, 9, 12, 15)
TAGS = tuple("t30k%d" % kx for kx in COUNTS)
IX, IL = 96, 48
# per count: moist.grid_inputs, radiation.columns, surface.columns of the fixture; the GPU tests' surface.columns / chain states
MOIST_SEED = {kx: 7100 + kx for kx in COUNTS}
RAD_SEED = {kx: 8100 + kx for kx in COUNTS}
SFC_SEED = {kx: 8200 + kx for kx in COUNTS}
CHAIN_SEED = {kx: 9700 + kx for kx in COUNTS}
THRESHOLD_COUNT, THRESHOLD_SEED = 12, 8312
# physstep.Case: (dynstep.state seed, moist.state seed, boundary seed) of the counts that run from spectra
CASE_SEEDS = {6: (8000, 5156, 31006), 12: (8000, 5162, 31012)}
# Three consecutive steps of the seeded 12-level state with the whole physics (see physstep.DT): at 300 s and 150 s the third step
# leaves temperatures of 1e7 K and 22 K, at 100 s of 103 K; at 50 s the state stays where it started (137 .. 302 K on the grid) and
# the smallest margin of the three steps is 3.0e-9 (found with the reference side alone on the CPU)
DT = 50.0

_tables = {}


def kx_of(tag):
    return COUNTS[TAGS.index(tag)]


def hsg(kx):
    return levels.sigma(kx)


def tables(kx):
    if kx not in _tables:
        _tables[kx] = moist.tables(hsg(kx))
    return _tables[kx]


def plan(kx, max_batch=64, device=0):
    """the T30 plan of kx levels on hsg(kx); device = -1: a host plan"""
    return levels.plan("t30", kx, max_batch, device)


def variant(tag):
    """(ix, il, kx, half levels, the reference has its own set) of a tag of support.PHYSICS_TAGS or of TAGS"""
    if tag in TAGS:
        kx = kx_of(tag)
        return IX, IL, kx, hsg(kx), False
    ix, il, kx = support.grid(tag)
    return ix, il, kx, moist.HSG[kx], kx != 16


def levels_case(kx, max_batch=None):
    """(plan, oracle, half levels, physstep.Case seeds) of a count of CASE_SEEDS: what physstep.plan_case takes as levels_case"""
    return plan(kx, max_batch or 4 * kx + 4), levels.oracle("t30", kx), hsg(kx), CASE_SEEDS[kx]
