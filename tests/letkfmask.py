"""What the member-mask tests share (include/spdy.h, "member mask"): a masked analysis of E members next to the
unmasked analysis of an object of the n members in use on the compacted ensemble, which the mask's definition says it equals bit
for bit, and the comparisons of the two."""
import numpy as np

import letkf as lk
import support

OBS_FIELDS = ("hxmean", "departure", "obs_lnsigma", "obs_used")


def flags(E, keep):
    """the mask of E entries with the members `keep` in use"""
    return [1 if e in set(keep) else 0 for e in range(E)]


def zero_bits(a):
    """every value is +0.0"""
    return not np.ascontiguousarray(a).view(np.int64).any()


def same_as_compact(got, ref, E, keep, tag=""):
    """the masked call `got` of E members against the unmasked call `ref` of the object of the members `keep`: the increments, y and
    hx at those members, the per-observation fields and members_used bit for bit; exactly 0.0 for the other members"""
    keep = list(keep)
    drop = [e for e in range(E) if e not in keep]
    for v in lk.VARS:
        assert support.same_bits(np.ascontiguousarray(got[v][keep]), ref[v]), (tag, v)
        assert ref[v].any(), (tag, v)
        assert zero_bits(got[v][drop]), (tag, v)
    if "y" in ref:
        for n in ("y", "hx"):
            assert support.same_bits(np.ascontiguousarray(got[n][:, keep]), ref[n]), (tag, n)
        assert zero_bits(got["y"][:, drop]), tag
        for n in OBS_FIELDS:
            assert support.same_bits(got[n], ref[n]), (tag, n)
    assert got["members_used"].tolist() == [float(len(keep))] == ref["members_used"].tolist(), tag


def pair(sp, g, E, keep, obs_of, sigma_v, seed=None, make=lk.make, ensemble=lk.ensemble, stride=None):
    """-> (x, obs, the object of E members, the object of len(keep) members, the compacted ensemble); obs_of(g, compacted x)"""
    x = ensemble(g, E, seed=E if seed is None else seed)
    xc = lk.compact(x, keep)
    obs = obs_of(g, xc)
    lt, ltc = make(sp, E, obs, sigma_v), make(sp, len(keep), obs, sigma_v)
    if stride is not None:
        lt.set_weight_stride(*stride)
        ltc.set_weight_stride(*stride)
    return x, obs, lt, ltc, xc
