"""ctypes binding of the gfx950 rasterizer library (C ABI: include/gs_raster.h).

The library is built ahead of time by `make -C easy_gaussian_splatting_amd/csrc`
(`__graft_entry__.build()` does that) and lives IN-TREE next to this file.  There is no
fallback: if the shared object is missing or a stage fails, the call raises.
"""
from __future__ import annotations

import ctypes as ct
import os
import subprocess
import threading
from typing import Optional

from ._header import parse as parse_header

_HERE = os.path.dirname(os.path.abspath(__file__))
# The product loads the in-tree build.  GS_LIB_PATH names another build of the same library -- a diagnostic VARIANT
# (`build_variant`: -DGS_BWD_CHECK, -DGS_BWD_ACC64, -DGS_EXACT_MATH, -DGS_CLOCK_PROBE, tuning constants) -- and is honoured only
# together with GS_ALLOW_VARIANT=1: every library names the flags it was built with (`gs_build_flags`), and one whose flags
# are not empty is refused otherwise, so that a stray environment variable cannot put a timing or checking build behind
# the numbers and the parity results.
LIB_PATH = os.environ.get("GS_LIB_PATH") or os.path.join(_HERE, "libgsraster.so")
CSRC_DIR = os.path.join(_HERE, "csrc")
VARIANT_DIR = os.path.join(os.path.dirname(_HERE), "build", "variants")   # never the package directory
HEADER_PATH = os.path.abspath(os.path.join(_HERE, "..", "include", "gs_raster.h"))

_lib: Optional[ct.CDLL] = None
_lock = threading.Lock()


class NativeLibraryError(RuntimeError):
    pass


def _read_header() -> str:
    try:
        with open(HEADER_PATH) as f:
            return f.read()
    except OSError as e:
        raise NativeLibraryError(f"{HEADER_PATH} cannot be read ({e.strerror}): the binding of libgsraster.so is derived from that "
                                 "header and there is no second copy of the ABI") from None


# The header is the one description of the ABI.  SIGNATURES: name -> (restype, [argtypes]) and PARAMS: name -> [parameter names]
# of every gs_* entry point it declares; DEFINES: every integer #define, each also a constant of this module (nat.GS_TILE,
# nat.GS_FLAG_ROWS, nat.GS_INFO_FLAGS, nat.GS_WS_REC, ...).
SIGNATURES, PARAMS, DEFINES = parse_header(_read_header())
globals().update(DEFINES)


def build(verbose: bool = False, clean: bool = False) -> str:
    """Compile the HIP sources for gfx950 with hipcc (cross-compiles without a GPU).  `clean`: from scratch -- no object of an
    earlier build (another revision, other flags) can end up in the library."""
    if clean:
        subprocess.run(["make", "-C", CSRC_DIR, "clean"], capture_output=True, text=True)
    proc = subprocess.run(["make", "-C", CSRC_DIR, "-j4"], capture_output=True, text=True)
    if verbose or proc.returncode != 0:
        print(proc.stdout)
        print(proc.stderr)
    if proc.returncode != 0:
        raise NativeLibraryError("building libgsraster.so failed:\n" + proc.stderr[-4000:])
    return LIB_PATH


def build_variant(name: str, extra_flags: str) -> str:
    """A diagnostic variant of the library, `build/variants/libgsraster_<name>.so` (outside the package), compiled with
    additional flags from a scratch copy of the sources (so the product's objects are left alone).  It reports those flags
    through `gs_build_flags`; a process loads it through GS_LIB_PATH + GS_ALLOW_VARIANT=1 (tests/test_gpu_contributors.py does,
    in a child process); never loaded by the package on its own."""
    import glob
    import shutil
    import tempfile
    os.makedirs(VARIANT_DIR, exist_ok=True)
    out = os.path.join(VARIANT_DIR, f"libgsraster_{name}.so")
    srcs = [f for pat in ("*.hip", "*.h", "*.inc", "Makefile") for f in glob.glob(os.path.join(CSRC_DIR, pat))]
    if os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(f) for f in srcs + [HEADER_PATH]):
        return out
    d = tempfile.mkdtemp(prefix=f"gsvar_{name}_")
    try:
        for f in srcs:
            text = open(f).read().replace("../../include/gs_raster.h", HEADER_PATH)
            open(os.path.join(d, os.path.basename(f)), "w").write(text)
        proc = subprocess.run(["make", "-C", d, "-j4", f"EXTRA={extra_flags}", f"LIB={out}"], capture_output=True, text=True)
        if proc.returncode != 0:
            raise NativeLibraryError(f"building {out} failed:\n" + proc.stderr[-4000:])
    finally:
        shutil.rmtree(d, ignore_errors=True)
    return out


def bind(cdll, names=None):
    """Types the entry points `names` (default: all the header declares) of a loaded library as the header declares them."""
    for name in SIGNATURES if names is None else names:
        fn = getattr(cdll, name)  # AttributeError => header/library mismatch
        fn.restype, fn.argtypes = SIGNATURES[name]
    return cdll


def lib() -> ct.CDLL:
    """Load (once) and return the native library; raises if it is not built."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise NativeLibraryError(
                        f"{LIB_PATH} is missing: the HIP rasterizer has not been built. Run "
                        "`python -c 'import __graft_entry__ as g; g.build()'` or "
                        f"`make -C {CSRC_DIR}`. There is no CPU fallback.")
                L = bind(ct.CDLL(LIB_PATH))
                flags = L.gs_build_flags().decode("utf-8", "replace")
                if flags and os.environ.get("GS_ALLOW_VARIANT") != "1":
                    raise NativeLibraryError(
                        f"{LIB_PATH} is a diagnostic variant of the rasterizer library (built with `{flags}`), not the product "
                        "build: refusing to run on it.  Unset GS_LIB_PATH, or set GS_ALLOW_VARIANT=1 if that is what you want.")
                _lib = L
    return _lib


def build_flags() -> str:
    """The extra preprocessor flags the loaded library was built with ("" = the product build)."""
    return lib().gs_build_flags().decode("utf-8", "replace")


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = lib().gs_last_error().decode("utf-8", "replace")
        if rc == -1:
            raise ValueError(f"{what}: {msg}")
        raise NativeLibraryError(f"{what} failed (code {rc}): {msg}")
