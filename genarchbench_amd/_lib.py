"""Loader for libgab_hip.so.  Fails loudly when the library is missing: there is no CPU fallback."""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.environ.get("GAB_LIB_PATH") or os.path.join(_HERE, "libgab_hip.so")   # override: A/B builds while tuning
_lib = None


class GabError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libgab_hip error {code}: {msg}")
        self.code = code


def build(force=False):
    """compile every HIP translation unit for gfx950 into genarchbench_amd/libgab_hip.so (in-tree)"""
    csrc = os.path.join(_HERE, "csrc")
    args = ["make", "-C", csrc, "-s"]
    if force:
        subprocess.check_call(args + ["clean"])
    subprocess.check_call(args)
    return _SO


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_SO):
            raise ImportError(
                f"{_SO} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or make -C genarchbench_amd/csrc).  There is no CPU fallback.")
        # PyTorch wheels bundle their own libamdhip64.so.7; a process must hold ONE HIP runtime.  When torch is
        # installed, load it first so that libgab_hip.so binds to the runtime torch uses (same soname) -- otherwise
        # a later `torch.cuda` initialisation in the same process finds no GPU.  The C drivers never see torch.
        try:
            import torch  # noqa: F401
        except Exception:
            pass
        _lib = C.CDLL(_SO)
        _lib.gab_version.restype = C.c_char_p
        _lib.gab_last_error.restype = C.c_char_p
        _dbg_prototypes(_lib)
    return _lib


def _dbg_prototypes(so):
    """argument and result types of the gab_dbg_* entry points (include/gab.h, dbg section)"""
    P, I64, I32 = C.c_void_p, C.c_int64, C.c_int32
    so.gab_dbg_create.argtypes = [C.c_int, P]
    so.gab_dbg_destroy.argtypes = [P]
    so.gab_dbg_destroy.restype = None
    so.gab_dbg_reserve.argtypes = [P, I64, I64, I64]
    so.gab_dbg_room.argtypes = [P, P, P, P, P, I64, I64, C.c_int, P]
    so.gab_dbg_room.restype = I64
    so.gab_dbg_build.argtypes = [P, P, P, P, P, P, P, P, P, P, P, I64, P, P, I64, P, P, I64, P]
    so.gab_dbg_build_device.argtypes = [P, P, P, I64, P, P, P, P, P, I64, P, P, P, I64, P, P, I64, P, P, I64, P, P]
    so.gab_dbg_last_stats.argtypes = [P, P]
    so.gab_dbg_last_phases.argtypes = [P, P, P, P]
    so.gab_dbg_plan_regions.argtypes = [I32, I32, P, P, I64, I32, P, I64, P]


def version():
    return lib().gab_version().decode()


def check(rc):
    if rc != 0:
        raise GabError(rc, lib().gab_last_error().decode())
