"""The reference side of the ensemble output tests (include/spdy.h, "ensemble output"): per member the FP64 grids of the oracle -- u, v
from uvspec followed by spec_to_grid(., 2), the rest from spec_to_grid(., 1) -- converted with the expressions of
input_output.f90:200-206, and over the members in use the mean and the ddof = 1 standard deviation in np.longdouble.  Member states
are dynstep.state with one seed per member (ensemblestep.member_states); phi is the oracle's geopotential of time level 1, an input
of the snapshot as in test_output_path."""
import numpy as np

import ensemblestep as es

FIELDS = ("u", "v", "t", "q", "phi", "ps")
QFAC, GRAV, P0 = float(np.float32(1.0e-3)), float(np.float32(9.81)), float(np.float32(1.0e5))   # float32 literals widened


def member_inputs(o, st):
    """time level 1 of one member as the output calls take it: vor, div, t, q (kx, nx, mx), phi, ps"""
    return [st["vor"][0], st["div"][0], st["t"][0], st["tr"][0], o.geopotential(st["t"][0], st["phis"]), st["ps"][0]]


def member_values(o, ins):
    """x_e of one member in FP64: {u, v, t, q, phi: (kx, il, ix), ps: (il, ix)}"""
    vor, div, t, q, phi, ps = ins
    uv = [o.uvspec(vor[k], div[k]) for k in range(o.kx)]
    plain = lambda a: np.stack([o.spec_to_grid(a[k], 1) for k in range(o.kx)])
    return {"u": np.stack([o.spec_to_grid(a, 2) for a, _ in uv]), "v": np.stack([o.spec_to_grid(b, 2) for _, b in uv]),
            "t": plain(t), "q": plain(q) * QFAC, "phi": plain(phi) / GRAV, "ps": P0 * np.exp(o.spec_to_grid(ps, 1))}


def statistics(xs, use=None):
    """xs: the members' member_values; use: None or a sequence of flags.  -> (mean, spread, scale): mean and sample standard
    deviation over the members in use, formed in np.longdouble and given in float64, and max |x_e| over them per quantity"""
    inc = [x for e, x in enumerate(xs) if use is None or use[e]]
    mean, spread, scale = {}, {}, {}
    for n in FIELDS:
        a = np.stack([x[n] for x in inc]).astype(np.longdouble)
        mean[n] = a.mean(axis=0).astype(np.float64)
        spread[n] = (a.std(axis=0, ddof=1) if len(inc) > 1 else np.zeros(a.shape[1:])).astype(np.float64)
        scale[n] = float(np.max(np.abs(a)))
    return mean, spread, scale


def ordered(a):
    """float32 bits as integers that are ordered like the values: neighbouring floats differ by 1"""
    i = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def ulps(a, b):
    """largest distance of two float32 arrays in units in the last place"""
    return int(np.max(np.abs(ordered(a) - ordered(b))))


def within(dev, ref, scale, contract=1e-12):
    """(b)'s bound: |device - float32(ref)| <= contract * max|x| + one float32 ulp of the reference value, compared in FP64.
    -> the largest excess over the bound (<= 0: met)"""
    r32 = ref.astype(np.float32)
    bound = contract * scale + np.spacing(np.abs(r32)).astype(np.float64)
    return float(np.max(np.abs(dev.astype(np.float64) - r32.astype(np.float64)) - bound))


def build(sp, o, sts, phis=None):
    """the ensemble of the member states sts on the device, phi of time level 1 in ens.phi (phis: given (kx, nx, mx) arrays in place
    of the oracle's geopotential); -> (ens, [member_inputs])"""
    import torch
    ens = es.build(sp, sts)
    ins = [member_inputs(o, st) for st in sts]
    for e in range(len(sts)):
        if phis is not None:
            ins[e][4] = phis[e]
        ens.phi[e].copy_(torch.as_tensor(np.ascontiguousarray(ins[e][4], np.complex128)))
    return ens, ins


def host(res):
    """an Ensemble.output result as NumPy arrays"""
    return {g: {n: a.cpu().numpy() for n, a in d.items()} for g, d in res.items()}


def single_output(sp, ins):
    """spdy_output_batch_dev on one member's inputs -> {field: float32 array}"""
    import torch
    dev = [torch.from_numpy(np.ascontiguousarray(a, np.complex128)).cuda() for a in ins]
    outs = [torch.zeros((sp.kx, sp.il, sp.ix), dtype=torch.float32, device="cuda") for _ in range(5)]
    outs.append(torch.zeros((sp.il, sp.ix), dtype=torch.float32, device="cuda"))
    sp.output_batch_dev(*dev, *outs)
    torch.cuda.synchronize()
    return {n: a.cpu().numpy() for n, a in zip(FIELDS, outs)}
