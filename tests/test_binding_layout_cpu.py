"""CPU: the Python binding's structures and field table against include/spdy.h.  The header is the sole definition of the structs
that cross the C-ABI; a ctypes mirror with two members swapped would silently exchange two pointers.  The typedef blocks of the
header are parsed here (members in order, their C type, the shape their comment gives) and compared with the ctypes structures,
with the dtypes of speedy.f90_amd/columns.py's FIELDS and with the public name tuples, which are also spelled out as literals."""
import ctypes
import re

import numpy as np
import pytest

import speedy_f90_amd as s
import support
from speedy_f90_amd import columns, spectral

MIRRORS = {"spdy_moist_out": spectral.MoistOut, "spdy_rad_surface": spectral.RadSurface, "spdy_rad_out": spectral.RadOut,
           "spdy_sfc_boundary": spectral.SfcBoundary, "spdy_sfc_out": spectral.SfcOut, "spdy_pbl_out": spectral.PblOut,
           "spdy_column_physics_out": spectral.ColumnPhysicsOut, "spdy_surface_clim": spectral.SurfaceClim,
           "spdy_spec_seg": spectral.SpecSeg, "spdy_step_op": spectral.StepOp, "spdy_hdiff_op": spectral.HdiffOp}
SHAPE = re.compile(r"\(ix,il(?:,(\w+))?\)")


def _shape(comment):
    """"kx", "3", ... for (ix,il,kx), (ix,il,3); "" for (ix,il); None without a shape"""
    m = SHAPE.search(comment or "")
    return None if m is None else (m.group(1) or "")


def parse_header(text):
    """{struct: [(member, C type ("double", "int", "spdy_x"), is a pointer, shape, comment), ...]} of the anonymous typedef structs"""
    out = {}
    for head, body, name in re.findall(r"typedef struct \{([^\n]*)\n(.*?)\}\s*(spdy_\w+);", text, re.S):
        default, members = _shape(head), []
        for ctype, decl, comment in re.findall(r"^\s*(?:const\s+)?(double|int|spdy_\w+)\s+([^;]+);[ \t]*(?:/\*(.*?)\*/)?", body, re.M | re.S):
            shape = _shape(comment)
            for m in decl.split(","):
                m = m.strip()
                members.append((m.lstrip("* "), ctype, m.startswith("*"), default if shape is None else shape, comment or ""))
        out[name] = members
    return out


@pytest.fixture(scope="module")
def header():
    return parse_header(support.header(comments=True))


def test_parser_reads_every_mirrored_struct(header):
    assert set(MIRRORS) <= set(header), sorted(set(MIRRORS) - set(header))
    assert [m[:4] for m in header["spdy_hdiff_op"]] == [("nlev", "int", False, None), ("field", "double", True, None),
                                                        ("fdt_in", "double", True, None), ("d_dmp", "double", True, None),
                                                        ("d_dmp1", "double", True, None), ("fdt_out", "double", True, None)]
    assert [m[:4] for m in header["spdy_moist_out"]][3:6] == [("iptop", "int", True, ""), ("icnv", "int", True, ""),
                                                              ("qsat", "double", True, "kx")]


@pytest.mark.parametrize("struct", sorted(MIRRORS))
def test_structure_members_in_header_order(header, struct):
    """same member names in the same order; pointers are c_void_p, plain ints c_int, nested structs their own mirror"""
    fields = MIRRORS[struct]._fields_
    assert [f[0] for f in fields] == [m[0] for m in header[struct]]
    for (name, ftype), (_, ctype, pointer, _, _) in zip(fields, header[struct]):
        want = ctypes.c_void_p if pointer else ctypes.c_int if ctype == "int" else MIRRORS[ctype]
        assert ftype is want, (struct, name, ftype)


def test_table_dtypes_and_shapes(header):
    """every `int *` member is int32 in the table and every `double *` member float64; the table's shape is the comment's"""
    seen = 0
    for struct, members in header.items():
        if struct not in MIRRORS or struct in ("spdy_spec_seg", "spdy_step_op", "spdy_hdiff_op"):
            continue
        for name, ctype, pointer, shape, _ in members:
            if not pointer:
                continue
            seen += 1
            assert columns.dtype_of(name) is (np.int32 if ctype == "int" else np.float64), (struct, name)
            lead = () if shape == "" else (5,) if shape == "kx" else (int(shape),)
            assert columns.shape_of(name, (2,), 5, (48, 96)) == (2,) + lead + (48, 96), (struct, name, shape)
    assert seen == 8 + 2 + 11 + 7 + 10 + 4 + 2 + 8
    assert [n for t in columns.FIELDS.values() for n, _, dt in t if dt is np.int32] == ["iptop", "icnv", "icltop"]


def test_public_tuples(header):
    """the tuples as literals (today's contents, in order), and as the header's members of each shape"""
    want = {"MOIST_2D": ("precnv", "precls", "cbmf", "iptop", "icnv"), "MOIST_3D": ("qsat", "rh", "se"),
            "RAD_SW_2D": ("cloudc", "clstr", "icltop", "ssrd", "ssr", "tsr"), "RAD_2D": ("slrd", "slr", "olr"),
            "RAD_3D": ("tt_rsw", "tt_rlw"), "SFC_BOUNDARY": ("fmask", "sst", "stl", "soilw", "snowc", "alb_l", "alb_s"),
            "SFC_3": ("ustr", "vstr", "shf", "evap", "slru"), "SFC_2D": ("tskin", "u0", "v0", "t0"), "PBL_2D": ("ut_pbl", "vt_pbl"),
            "PBL_3D": ("tt_pbl", "qt_pbl")}
    for name, members in want.items():
        assert getattr(spectral, name) == members and getattr(columns, name) == members, name

    def of(struct, shape, sw=None):
        return tuple(m[0] for m in header[struct] if m[3] == shape and (sw is None or ("compute_sw calls only" in m[4]) == sw))
    assert of("spdy_moist_out", "") == want["MOIST_2D"] and of("spdy_moist_out", "kx") == want["MOIST_3D"]
    assert of("spdy_rad_out", "", True) == want["RAD_SW_2D"] and of("spdy_rad_out", "", False) == want["RAD_2D"]
    assert of("spdy_rad_out", "kx") == want["RAD_3D"]
    assert of("spdy_sfc_boundary", "") == want["SFC_BOUNDARY"] == tuple(m[0] for m in header["spdy_sfc_boundary"])
    assert of("spdy_sfc_out", "3") == want["SFC_3"] and of("spdy_sfc_out", "2") == ("hfluxn",) and of("spdy_sfc_out", "") == want["SFC_2D"]
    assert of("spdy_pbl_out", "") == want["PBL_2D"] and of("spdy_pbl_out", "kx") == want["PBL_3D"]


def test_import_paths():
    """the names the package and the spectral module exported before the column physics moved to columns.py"""
    for n in ("RESOLUTIONS", "DeviceField", "Graph", "Spectral", "SurfaceModel", "check", "LIB_PATH", "SpdyError", "build", "load",
              "sharding"):
        assert hasattr(s, n), n
    for n in ("SurfaceModel", "DeviceField", "SurfaceClim", "SURFACE_LAND_COUPLING", "SURFACE_ICE_COUPLING", "SURFACE_SST_ANOMALY",
              "SURFACE_DEFAULT", "SURFACE_TABLES", "SURFACE_FIELDS", "Graph", "Spectral"):
        assert hasattr(spectral, n), n
    assert issubclass(spectral.Spectral, columns.ColumnPhysics)
