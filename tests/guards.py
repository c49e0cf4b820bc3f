"""Guard bands, per-field error and the launchers' route predicates, for the measured-path tests (test_gpu_measured_path.py).

Every output a guarded test checks is a view into one larger allocation, with at least one whole field of sentinel bits
before it, after it and between the outputs of one call.  The sentinel is a fixed int64 pattern (a finite double), so a
stray store of anything -- NaN included -- changes it.  The outputs themselves start as NaN, so a field that is never
written fails the reference check.
"""
import os

import numpy as np

SENTINEL = 0x5A5AA5A5C3C33C3C    # exponent 0x5A5: a finite double (about 1e127), far from any value these tests produce
MIB = 1 << 20


class Guarded:
    """One device allocation holding `len(counts)` outputs of `counts[i]` fields of `field_shape` each (complex: complex128
    fields), laid out as  [pad] out0 [pad] out1 ... [pad]  with `pad` whole fields of sentinel bits in every gap."""

    def __init__(self, torch, field_shape, counts, complex_=False, pad=1, device="cuda"):
        self.torch, self.complex = torch, complex_
        shape = tuple(field_shape) + ((2,) if complex_ else ())
        total = sum(counts) + pad * (len(counts) + 1)
        self.base = torch.empty((total,) + shape, dtype=torch.float64, device=device)
        self.base.view(torch.int64).fill_(SENTINEL)
        self.outs, self.bands = [], []
        at = 0
        for n in counts:
            self.bands.append((at, at + pad))
            at += pad
            v = self.base[at:at + n]
            self.outs.append(torch.view_as_complex(v) if complex_ else v)
            at += n
        self.bands.append((at, at + pad))
        self.fill_nan()

    def fill_nan(self):
        for o in self.outs:
            o.fill_(float("nan"))

    def intact(self):
        """True when every sentinel field still holds the pattern, bit for bit."""
        return all(bool((self.base[a:b].view(self.torch.int64) == SENTINEL).all()) for a, b in self.bands)

    def hits(self):
        """(band index, field offset in the band) of every sentinel field that changed -- for the failure message."""
        out = []
        for i, (a, b) in enumerate(self.bands):
            bad = (self.base[a:b].view(self.torch.int64) != SENTINEL).flatten(1).any(1).nonzero().flatten().tolist()
            out += [(i, j) for j in bad]
        return out


def field_err(torch, got, ref):
    """Per-field  max|got - ref| / max|ref|  (synth.relerr of each field) over the leading axis, as a NumPy array; NaN in
    `got` gives NaN for that field.  got / ref: tensors of one shape on one device (complex compared by modulus)."""
    d = (got - ref).abs().flatten(1).amax(1)
    s = ref.abs().flatten(1).amax(1)
    return torch.where(s > 0, d / torch.where(s > 0, s, torch.ones_like(s)), d).cpu().numpy()


def worst(err):
    """(index, value) of the worst field; a NaN field counts as the worst."""
    e = np.where(np.isnan(err), np.inf, err)
    i = int(np.argmax(e))
    return i, float(err[i])


# ---------------------------------------------------------------------------------------------------------------- routes
# The launchers' choice of kernel form, restated (csrc/spdy_fused_t30.inc: stream_policy, write_through_policy,
# launch_s2g_fused, launch_g2s_fused; csrc/spdy_fused_t63.inc: launch_s2g_fused_t63_batch, g2s_t63_staged,
# launch_g2s_fused_t63_batch).  Default launch options (the tests pin them with set_option).
STREAM_MIN = 16 * MIB        # grid-side bytes of a launch from which it streams (non-temporal stores)
WT_MIN = 6 * MIB             # output bytes from which a T63 by-chunk inverse writes through (wt_min_mb = 6)
GRID_BYTES = {"t30": 48 * 96 * 8, "t63": 96 * 192 * 8}


def max_wg(tag, num_cu):
    """Workgroups of the persistent launches: T30 num_cu x SPDY_WG_PER_CU (plan creation reads it), T63 num_cu."""
    if tag == "t63":
        return num_cu
    try:
        per = int(os.environ.get("SPDY_WG_PER_CU", "1"))
    except ValueError:
        per = 1
    return num_cu * max(per, 1)


def route(tag, direction, nb, num_cu, pairs=False, max_batch=None):
    """Kernel form of ONE fused launch over nb plain fields (pairs=False) or nb (u, v) / (vor, div) pairs, direction "s2g"
    (inverse) or "g2s" (direct):
        T30 s2g: "part" (three workgroups per tile), "stream", "resident"
        T30 g2s: "split" (three workgroups per tile), "stream", "resident"
        T63 s2g: "chunk_wt" / "chunk" (one (pair, chunk) item per workgroup step, written through or not), "stream", "resident"
        T63 g2s: "staged" (row FFTs, then the contraction), "split" (two workgroups per pair), "stream", "resident"
    A T30 tile is 2 plain fields or 1 pair; a T63 work unit is a field pair (pairs: two segments of nb fields, 2 ceil(nb/2) units)."""
    fields = 2 * nb if pairs else nb
    if tag == "t30":
        return route_units(tag, direction, nb if pairs else (nb + 1) // 2, fields, num_cu)
    units = 2 * ((nb + 1) // 2) if pairs else (nb + 1) // 2     # T63 pairs: one segment per member, each (nb + 1) / 2 units
    # (vdspec: the staged form takes the pairs as ONE segment)
    return route_units(tag, direction, units, fields, num_cu, staged_units=nb if pairs else units, max_batch=max_batch)


def route_units(tag, direction, units, fields, num_cu, staged_units=None, max_batch=None):
    """route() for a launch given by its work units (T30 tiles, T63 field pairs) and the fields of grids it reads or writes --
    what a mixed launch (pairs, plain segments and a gradient together) comes to.  staged_units: the units of the T63 direct
    launch as the staged form would take it (vdspec pairs one unit each), where that differs."""
    nwg = max_wg(tag, num_cu)
    gbytes = fields * GRID_BYTES[tag]
    stream = gbytes >= STREAM_MIN
    if tag == "t30":
        tiles = units
        if direction == "s2g":
            return "part" if 3 * tiles <= nwg and not stream else "stream" if stream else "resident"
        return "split" if 6 * tiles <= nwg and not stream else "stream" if stream else "resident"
    if direction == "s2g":
        if 2 * units <= nwg:
            return "chunk_wt" if gbytes >= WT_MIN else "chunk"
        return "stream" if stream else "resident"
    rows_ws = min(3 * max_batch + 2, 258)                        # the plan's row workspace (csrc/spdy_api.hip, upload_all)
    staged = lambda u: 2 * u <= rows_ws and 3 * u <= nwg
    if staged(units if staged_units is None else staged_units):
        return "staged"
    if 2 * units <= nwg:
        return "split"
    return "stream" if stream else "resident"


def mixed_units(tag, direction, npairs, plain, ngrad=0):
    """(units, fields, staged_units) of ONE mixed launch for route_units: npairs operator pairs, plain segments of `plain` fields
    each (a tuple; the direct batch has one) and ngrad gradients (csrc/spdy_api.hip: inverse_batch, direct_batch).  T30 tiles: a
    pair or a gradient each, two plain fields of the concatenated segments.  T63 units: pairs formed inside each segment -- the
    operator pairs and the gradient are two segments each; the staged direct form takes the (u, v) pairs as one unit each."""
    half = lambda n: (n + 1) // 2
    fields = 2 * (npairs + ngrad) + sum(plain)
    if tag == "t30":
        return npairs + ngrad + half(sum(plain)), fields, None
    units = 2 * half(npairs) + 2 * half(ngrad) + sum(half(n) for n in plain)
    return units, fields, (npairs + sum(half(n) for n in plain) if direction == "g2s" else None)


def pin_launch_options(sp):
    """The launch options at their defaults, whatever the environment set when the plan was made."""
    for name, value in (("t30_part", 1), ("t30_split", 1), ("t63_split", 1), ("t63_stage", 1), ("t63_derive", 1), ("wt_min_mb", 6)):
        sp.set_option(name, value)


# ------------------------------------------------------------------------------------------------------- per-column error
def column_err(got, ref, scale=None):
    """Per-column error of a column-physics output [.., ncol] or [ncol] (NumPy): max over the leading axes of |got - ref| divided
    by the column's own scale -- max|ref| of the column, or where `scale` is given (the output is a difference of large terms, and
    the scale has to come from its operands) the larger of the two; scale is [ncol], or shaped like ref where the operands differ
    from level to level.  Columns are independent and span orders of magnitude, so one number per array (synth.relerr) hides a
    small column that is wrong.  Where the reference is exactly 0 in a whole column (no convection, polar night, nothing above
    level kx), the device must be exactly 0 there: any other value gives inf.  NaN in `got` gives inf."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    n = ref.shape[-1]
    d = np.abs(got - ref).reshape(-1, n)
    own = np.max(np.abs(ref).reshape(-1, n), axis=0)
    s = np.broadcast_to(own, d.shape) if scale is None else np.maximum(np.broadcast_to(np.asarray(scale, np.float64), ref.shape).reshape(-1, n), own)
    dmax = np.max(d, axis=0)
    e = np.max(np.where(s > 0, d / np.where(s > 0, s, 1.0), np.where(d > 0, np.inf, 0.0)), axis=0)
    e = np.where((own == 0) & (dmax > 0), np.inf, e)
    return np.where(np.isnan(e), np.inf, e)
