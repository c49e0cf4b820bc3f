"""speedy.f90_amd -- MI355X-native grid<->spectral transform path for speedy.f90.

Only what the hot path needs lives here:
    csrc/      HIP kernels (gfx950) + the C-ABI (include/spdy.h) + host table generation
    fortran/   ISO_C_BINDING drop-in for the reference's `spectral` module (the real host)
    spectral.py  Python mirror of that module over the same C-ABI (ctypes), used by tests,
                 smoke() and bench.py
    columns.py   the column physics and the surface models of the same plan: one field table,
                 the ctypes structures and output buffers derived from it
    ensemble.py  E model states through one time step's launches: the layout, the views, the step
    letkf.py     the ensemble analysis: observations in, the LETKF update of all members on the device
    nature.py    the nature run of a twin experiment: the truth, observations drawn from it, an ensemble's scores against it

The directory name contains a dot, so import it through the repo-root shim
``import speedy_f90_amd`` (speedy_f90_amd.py).
"""
from ._lib import LIB_PATH, SpdyError, build, load  # noqa: F401
from .spectral import (RESOLUTIONS, DeviceField, Diagnostics, DiagnosticsStop, Graph, Spectral, Sppt, SurfaceModel,  # noqa: F401
                       check)
from .ensemble import Ensemble  # noqa: F401
from .letkf import OBS_AT_P, OBS_PS, OBS_Q, OBS_T, OBS_U, OBS_V, Letkf, PObs  # noqa: F401
from .nature import Nature  # noqa: F401
from . import sharding  # noqa: F401
