"""The visible Adam step, host side: gs_adam_step_visible / gs_adam_step_visible_dev / gs_project_bwd_selective are declared, bound and
exported, refuse bad arguments before anything is launched, and the selective fused instantiations keep the scratch-free allocation and
the occupancy of the dense ones -- no GPU."""
import ctypes as ct
import os
import re

import pytest


@pytest.fixture(scope="module")
def native():
    from easy_gaussian_splatting_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    return _native


NEW = ("gs_adam_step_visible", "gs_adam_step_visible_dev", "gs_project_bwd_selective")


def test_new_symbols_are_declared_bound_and_exported(native):
    hdr = open(native.HEADER_PATH).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = native.lib()
    for n in NEW:
        assert re.search(r"\b" + n + r"\s*\(", hdr), f"{n} not declared in include/gs_raster.h"
        assert n in native.SIGNATURES, f"{n} missing from the ctypes signature table"
        assert hasattr(lib, n)
    S = native.SIGNATURES
    tail = [ct.c_int64, ct.c_void_p, ct.c_void_p]   # n_rows, seg_widths_host, radii
    assert S["gs_adam_step_visible"][1] == S["gs_adam_step"][1] + tail
    assert S["gs_adam_step_visible_dev"][1] == S["gs_adam_step_dev"][1] + tail
    assert S["gs_project_bwd_selective"][1] == S["gs_project_bwd_adam"][1] + [ct.c_int, ct.c_float, ct.c_float]
    assert native.PARAMS["gs_project_bwd_selective"][-3:] == ["reg_on", "max_ratio", "lambda"]
    # tests/test_stage_calls_host.py holds every entry of this prefix to the table of tests/fused_variants.py: the new one stands outside
    assert not "gs_project_bwd_selective".startswith("gs_project_bwd_adam")
    assert not [n for n in S if n.startswith("gs_project_bwd_adam") and "selective" in n]


def _step_args(n_rows=5, widths=(3, 4, 0, 1)):
    """Host-side arguments of a well-formed call over fake (never dereferenced) device addresses."""
    ns = len(widths)
    lens = [n_rows * w for w in widths]
    ends, off = [], 0
    for n in lens:
        off = (off + n + 3) // 4 * 4
        ends.append(off)
    keep = dict(ends=(ct.c_int64 * ns)(*ends), lens=(ct.c_int64 * ns)(*lens), grads=(ct.c_void_p * ns)(*[0x1000 * (k + 1) for k in range(ns)]),
                lrs=(ct.c_float * ns)(*[1e-3] * ns), widths=(ct.c_int64 * ns)(*widths))
    return off, ns, keep


def _host(L, keep, n, ns, n_rows, radii=0x9000, p=0x100, widths="widths", lens="lens"):
    return L.gs_adam_step_visible(None, n, p, 0x200, 0x300, ns, keep["ends"], keep[lens], keep["grads"], keep["lrs"], 0.9, 0.999, 1e-8, 1, 1.0,
                                  n_rows, keep[widths] if widths else None, radii)


def _dev(L, keep, n, ns, n_rows, radii=0x9000, hyper=0x400, widths="widths"):
    return L.gs_adam_step_visible_dev(None, n, 0x100, 0x200, 0x300, ns, keep["ends"], keep["lens"], keep["grads"], 0.9, 0.999, 1e-8, 1.0, hyper,
                                      None, n_rows, keep[widths] if widths else None, radii)


def test_visible_step_argument_checks(native):
    """Every refusal fires on the host, in front of the launch (the addresses are fake: a launch would fault)."""
    L = native.lib()
    n, ns, keep = _step_args()
    for call in (_host, _dev):
        assert call(L, keep, n, ns, 5, radii=None) == -1
        assert b"null pointer" in L.gs_last_error()
        assert call(L, keep, n, ns, 5, widths=None) == -1
        assert b"null pointer" in L.gs_last_error()
        assert call(L, keep, n, ns, -1) == -1
        assert b"n_rows >= 0" in L.gs_last_error()
        assert call(L, keep, n, ns, 6) == -1   # a length that is not n_rows * width
        assert b"n_rows * seg_widths" in L.gs_last_error()
        assert call(L, keep, n, ns, 5, radii=0x9002) == -1
        assert b"4-byte" in L.gs_last_error()
        # nothing to do: no device touched, whatever the device pointers are
        assert call(L, keep, 0, ns, 5, radii=None) == 0
        assert call(L, keep, n, ns, 0, radii=None) == 0
    assert _host(L, keep, n, ns, 5, p=None) == -1
    assert b"null pointer" in L.gs_last_error()
    assert _dev(L, keep, n, ns, 5, hyper=None) == -1
    assert b"hyper_dev" in L.gs_last_error()
    bad = dict(keep, widths=(ct.c_int64 * ns)(3, 4, -1, 1))
    assert _host(L, bad, n, ns, 5) == -1
    assert b"segment widths" in L.gs_last_error()
    short = dict(keep, lens=(ct.c_int64 * ns)(15, 19, 0, 5))   # one segment a float short of its Gaussians
    assert _host(L, short, n, ns, 5) == -1
    assert b"n_rows * seg_widths" in L.gs_last_error()


def test_selective_fused_argument_checks(native):
    L = native.lib()
    offs = (ct.c_int64 * 6)(*range(6))
    # (a plain tuple literal: tests/test_native_header.py counts the call below against the header with it)
    args = (None, 8, 16, 3, None, None, None, offs, None, None, 32, 32, 0.3, 0.01, 1e10, None, None, None, None, None, None, None, None,
            0.9, 0.999, 1e-15, None, None, None, None, None, None)
    assert L.gs_project_bwd_selective(*args, 1, 2.0, 0.1) == -1
    assert b"null pointer" in L.gs_last_error()
    selective = L.gs_project_bwd_selective
    assert selective(*args, 2, 2.0, 0.1) == -1
    assert b"reg_on" in L.gs_last_error()
    bad_deg = list(args)
    bad_deg[3], bad_deg[2] = 5, 36
    assert selective(*bad_deg, 0, 0.0, 0.0) == -1
    assert b"degree" in L.gs_last_error()
    none = list(args)
    none[1] = 0   # N = 0: valid, nothing to launch
    assert selective(*none, 0, 0.0, 0.0) == 0


def test_selective_instantiations_keep_scratch_and_occupancy(native):
    """project_bwd_selective_kernel<D, REG>: no scratch and the waves per SIMD of project_bwd_kernel<D, true, false[, true]> at every degree."""
    csrc = native.CSRC_DIR
    res = os.path.join(csrc, "gs_project.res")
    if not os.path.exists(res):
        import subprocess
        subprocess.run(["make", "-C", csrc, "-B", "-j4"], check=True, capture_output=True)
    txt = open(res).read()
    pat = re.compile(r"Function Name: (\S+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+)", re.S)
    found = {m.group(1): (int(m.group(2)), int(m.group(3)), int(m.group(4))) for m in pat.finditer(txt)}
    for d in "01234":
        for reg in "01":
            sel = found[f"_ZN2gs28project_bwd_selective_kernelILi{d}ELi{reg}EEEvNS_11ProjBwdArgsE"]
            dense = found[f"_ZN2gs18project_bwd_kernelILi{d}ELb1ELb0ELb{reg}EEEvNS_11ProjBwdArgsE"]
            print(f"degree {d} reg {reg}: selective VGPRs {sel[0]} scratch {sel[1]} waves {sel[2]}; dense VGPRs {dense[0]} waves {dense[2]}")
            assert sel[1] == 0 and dense[1] == 0 and sel[2] == dense[2], (d, reg, sel, dense)
    adam = open(os.path.join(csrc, "gs_adam.res")).read()
    vis = {m.group(1): (int(m.group(3)), int(m.group(4))) for m in pat.finditer(adam) if "adam_step" in m.group(1)}
    assert any("adam_step_visible_kernel" in k for k in vis) and all(s == 0 for s, _ in vis.values()), vis
