"""The scale-ratio regulariser, host side: the entry points gs_scale_reg / gs_project_bwd_adam_reg are declared, bound and refuse bad
arguments before anything is launched, and the regularised fused instantiation keeps the occupancy of the plain one -- no GPU."""
import ctypes as ct
import glob
import os
import re

import pytest


@pytest.fixture(scope="module")
def native():
    from easy_gaussian_splatting_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    return _native


NEW = ("gs_scale_reg", "gs_scale_reg_workspace_floats", "gs_project_bwd_adam_reg")


def test_new_symbols_are_declared_bound_and_exported(native):
    hdr = open(os.path.join(os.path.dirname(native.CSRC_DIR), "..", "include", "gs_raster.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = native.lib()
    for n in NEW:
        assert re.search(r"\b" + n + r"\s*\(", hdr), f"{n} not declared in include/gs_raster.h"
        assert n in native.SIGNATURES, f"{n} missing from the ctypes signature table"
        assert hasattr(lib, n)
    # the fused sibling takes gs_project_bwd_adam's arguments plus (max_ratio, lambda)
    assert native.SIGNATURES["gs_project_bwd_adam_reg"][1] == native.SIGNATURES["gs_project_bwd_adam"][1] + [ct.c_float, ct.c_float]


def test_workspace_size(native):
    L = native.lib()
    assert L.gs_scale_reg_workspace_floats(0) == 2
    assert L.gs_scale_reg_workspace_floats(1) == 2 + 2
    assert L.gs_scale_reg_workspace_floats(256) == 2 + 2
    assert L.gs_scale_reg_workspace_floats(257) == 2 + 4
    assert L.gs_scale_reg_workspace_floats(1_000_000) == 2 + 2 * 3907


def test_scale_reg_argument_checks(native):
    L = native.lib()
    buf = (ct.c_float * 64)()
    base = ct.addressof(buf)
    al = (base + 15) & ~15   # 16-byte aligned inside the buffer
    ls, loss3, ws, v = al, al + 16, al + 32, al + 48
    assert L.gs_scale_reg(None, -1, ls, 2.0, 0.1, loss3, ws, v) == -1
    assert b"N >= 0" in L.gs_last_error()
    assert L.gs_scale_reg(None, 4, None, 2.0, 0.1, loss3, ws, v) == -1
    assert b"null" in L.gs_last_error()
    assert L.gs_scale_reg(None, 4, ls, 2.0, 0.1, loss3, None, v) == -1
    assert b"null" in L.gs_last_error()
    assert L.gs_scale_reg(None, 4, ls, 2.0, 0.1, loss3, ws + 4, v) == -1   # the fp64 partials: 16-byte aligned workspace
    assert b"16-byte" in L.gs_last_error()
    for bad in ((ls + 2, loss3, v), (ls, loss3 + 1, v), (ls, loss3, v + 2)):
        assert L.gs_scale_reg(None, 4, bad[0], 2.0, 0.1, bad[1], ws, bad[2]) == -1
        assert b"4-byte" in L.gs_last_error()
    # N = 0: valid, nothing to launch (no device touched)
    assert L.gs_scale_reg(None, 0, ls, 2.0, 0.1, None, ws, None) == 0


def test_fused_sibling_argument_checks(native):
    L = native.lib()
    offs = (ct.c_int64 * 6)(*range(6))
    args = [None, 8, 16, 3, None, None, None, offs, None, None, 32, 32, 0.3, 0.01, 1e10] + [None] * 8 + [0.9, 0.999, 1e-15, None, None,
                                                                                                       None, None, None, None]
    assert L.gs_project_bwd_adam_reg(*args, 2.0, 0.1) == -1
    assert b"null pointer" in L.gs_last_error()
    bad_deg = list(args)
    bad_deg[3] = 4
    assert L.gs_project_bwd_adam_reg(*bad_deg, 2.0, 0.1) == -1


def test_regularised_fused_instantiation_keeps_the_occupancy(native):
    """project_bwd_kernel<D, true, false, true> (gs_project_bwd_adam_reg): no scratch, 3 waves per SIMD like the plain fused form."""
    csrc = native.CSRC_DIR
    res = os.path.join(csrc, "gs_project.res")
    if not os.path.exists(res):
        import subprocess
        subprocess.run(["make", "-C", csrc, "-B", "-j4"], check=True, capture_output=True)
    txt = open(res).read()
    pat = re.compile(r"Function Name: (\S+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+)", re.S)
    found = {m.group(1): (int(m.group(2)), int(m.group(3)), int(m.group(4))) for m in pat.finditer(txt)}
    for d in ("0", "1", "2", "3"):
        reg = found[f"_ZN2gs18project_bwd_kernelILi{d}ELb1ELb0ELb1EEEvNS_11ProjBwdArgsE"]
        plain = found[f"_ZN2gs18project_bwd_kernelILi{d}ELb1ELb0ELb0EEEvNS_11ProjBwdArgsE"]
        assert reg[1] == 0 and reg[2] >= 3 and reg[2] == plain[2], (d, reg, plain)
    assert glob.glob(os.path.join(csrc, "gs_scale_reg.hip"))
