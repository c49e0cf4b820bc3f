"""What the ensemble SPPT tests share (tests/test_gpu_ensemble_sppt.py): seeds, the three device fields of a pattern object in the
members' layout, the single objects every member is compared with, and a stand-in that leaves an advance out of a step."""
import numpy as np

import sppt
import support

SEED = 0x5EED0123456789AB
FIELDS = ("eta", "spec", "pattern")
NSTEPS = sppt.NSTEPS


def seeds(nmem, base=SEED):
    """nmem distinct 64-bit seeds, far apart"""
    return [(base + 0x9E3779B97F4A7C15 * e) & 0xFFFFFFFFFFFFFFFF for e in range(nmem)]


def mu(kx):
    """a taper with 0, fractions and 1 in it"""
    m = np.clip(np.linspace(-0.5, 1.5, kx), 0.0, 1.0)
    assert m[0] == 0.0 and m[-1] == 1.0 and ((m > 0) & (m < 1)).any()
    return m


def shape(sp):
    return (sp.kx, sp.nx, sp.mx)


def fields(pat):
    """host copies of eta, spec, pattern with the members in front, [nmem, kx, ..], whatever nmem is"""
    out = {}
    for n in FIELDS:
        a = pat.numpy(n)
        out[n] = a if pat.nmem > 1 else a[None]
    return out


def singles(sp, seed_list, mu=None):
    import speedy_f90_amd as s
    return [s.Sppt(sp, NSTEPS, mu, seed=x) for x in seed_list]


def differing(got, e, one):
    """the fields where member e of the ensemble object's copies `got` is not bit-equal to the single object `one`"""
    want = fields(one)
    return [n for n in FIELDS if not support.same_bits(got[n][e], want[n][0])]


def injected(nmem, d, shp, scale=4.0, base=SEED + 7):
    """noise to inject at advance d, [nmem, kx, nx, mx], different per member, scaled so that both clips have work"""
    n = int(np.prod(shp))
    return np.stack([scale * sppt.raw_noise(base + 100 * e, d, n).reshape(shp) for e in range(nmem)])


class NoAdvance:
    """a pattern object as Ensemble.step sees it whose advance does nothing: the step then applies the previous pattern"""

    def __init__(self, pat):
        self.h, self.nmem = pat.h, pat.nmem

    def advance_dev(self, eta=None):
        pass
