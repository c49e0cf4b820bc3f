"""SPPT restated in NumPy: the reference side of tests/test_sppt_cpu.py and tests/test_gpu_sppt.py.

sppt.f90 and physics.f90:85-88, :207-222 as the reference writes them (float32 literals widened, its order of operations), with
the noise taken from the generator include/spdy.h defines (Philox4x32-10 and its mapping to two uniforms) in place of the
reference's random_number: tests/golden/ref_sppt.npz pins everything after the uniforms to the flang-built reference, which is
replayed there on recorded noise.  Arrays are NumPy C-order views of the reference's: a spectrum (mx,nx,kx) is [kx, nx, mx]."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
U32 = 0xFFFFFFFF
f32 = lambda x: np.float64(np.float32(x))
STDDEV, LEN_DECORR, TIME_DECORR, REARTH = f32(0.33), f32(500000.0), f32(6.0), f32(6.371e+6)
FOUR_PI = np.float64(np.float32(2.0) * np.float32(6.28318530718))       # randn's 2.0 * 6.28318530718 = 12.566370964050293
NSTEPS = 36                                                           # params.f90


def philox4x32_10(counter, key):
    """counter: four arrays (or integers) of 32-bit words, key: two; returns the four output words as uint64 arrays < 2**32"""
    c = [np.asarray(x, np.uint64) & np.uint64(U32) for x in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & U32, int(key[1]) & U32
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & np.uint64(U32), p1 >> np.uint64(32), p1 & np.uint64(U32)
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & U32, (k1 + W1) & U32
    return c


def uniforms(w):
    """(r1 in (0, 1], r2 in [0, 1)) of the output words w0..w3"""
    w = [np.asarray(x, np.uint64) for x in w]
    a = (w[0] >> np.uint64(5)) * np.uint64(1 << 26) + (w[1] >> np.uint64(6))
    b = (w[2] >> np.uint64(5)) * np.uint64(1 << 26) + (w[3] >> np.uint64(6))
    return (a.astype(np.float64) + 1.0) * 2.0 ** -53, b.astype(np.float64) * 2.0 ** -53


def randn(r1, r2):
    """sppt.f90:102-116 with mean 0 and stdev 1"""
    u = np.sqrt(f32(-2.0) * np.log(r1))
    return u * np.sin(FOUR_PI * r2)


def clip(x, lim):
    """min(lim, abs(x)) * sign(1.0, x) (sppt.f90:66-68, :98)"""
    return np.minimum(lim, np.abs(x)) * np.copysign(1.0, x)


def raw_noise(seed, draws, n):
    """the n complex draws of advance number `draws` (0-based) before the clip, in storage order"""
    key = (seed & U32, seed >> 32)
    idx = np.arange(n, dtype=np.uint64)
    parts = [randn(*uniforms(philox4x32_10((idx, part, draws & U32, draws >> 32), key))) for part in (0, 1)]
    return parts[0] + 1j * parts[1]


def noise(seed, draws, shape):
    """eta [kx, nx, mx] of advance number `draws`, clipped to +-10"""
    z = raw_noise(seed, draws, int(np.prod(shape)))
    return (clip(z.real, 10.0) + 1j * clip(z.imag, 10.0)).reshape(shape)


def tables(trunc, nsteps=NSTEPS):
    """phi, f0, first and sigma [nx, mx] (sppt.f90:32, :76-80, :84)"""
    mx, nx = trunc + 1, trunc + 2
    phi = np.exp(-(24 / np.float64(nsteps)) / TIME_DECORR)
    r2 = (LEN_DECORR / REARTH) ** 2
    s = np.float64(0.0)
    for n in range(1, trunc + 1):
        s = s + (2 * n + 1) * np.exp(-(f32(0.5) * r2 * n * (n + 1)))
    f0 = np.sqrt((STDDEV * STDDEV * (1 - phi * phi)) / (2 * s))
    l = np.arange(nx)[:, None] + np.arange(mx)[None, :]
    el2 = (l * (l + 1)).astype(np.float32).astype(np.float64) / (REARTH * REARTH)       # spectral.f90:36
    sigma = f0 * np.exp(-(f32(0.25) * LEN_DECORR * LEN_DECORR * el2))
    return {"phi": phi, "f0": f0, "first": (1 - phi * phi) ** np.float64(-0.5), "sigma": sigma}


class Pattern:
    """gen_sppt: spec and the clipped grid after each advance; o is the oracle (its spec_to_grid), eta the noise to use"""

    def __init__(self, o, nsteps=NSTEPS):
        self.o, self.tab, self.draws, self.spec = o, tables(o.trunc, nsteps), 0, None

    def advance(self, eta):
        t = self.tab
        eta = clip(eta.real, 10.0) + 1j * clip(eta.imag, 10.0)
        if self.draws == 0:
            c = t["first"] * t["sigma"]
            self.spec = c * eta.real + 1j * (c * eta.imag)
        else:
            self.spec = (t["phi"] * self.spec.real + t["sigma"] * eta.real) + 1j * (t["phi"] * self.spec.imag + t["sigma"] * eta.imag)
        self.draws += 1
        self.grid = np.stack([self.o.spec_to_grid(np.ascontiguousarray(s), 1) for s in self.spec])
        self.pattern = clip(self.grid, 1.0)
        return self.pattern


def apply(tend, tend_dyn, pattern, mu):
    """physics.f90:212-221 on [kx, ...] arrays"""
    mu = np.asarray(mu, np.float64).reshape((-1,) + (1,) * (tend.ndim - 1))
    return (1 + pattern * mu) * (tend - tend_dyn) + tend_dyn


def mu(kx):
    """a taper with 0, fractions and 1 in it"""
    m = np.clip(np.linspace(-0.5, 1.5, kx), 0.0, 1.0)
    assert m[0] == 0.0 and m[-1] == 1.0 and ((m > 0) & (m < 1)).any(), "the taper of %d levels lacks 0, a fraction or 1: %s" % (kx, m)
    return m
